"""Restatement of kmcf_current_map (include/kmcfield.h) in numpy: per node of the T matrix the current through it, its
tunnel share and its Kirchhoff residual, from a neighbour CSR, a tunnel CSR and a potential vector.  Nothing here calls
the library under test for a number; the builders below only fetch the device's own exports (pattern, values, tunnel
block) or an oracle.TSystem and hand them to the same restatement.

A pair is a stored off-diagonal (r, c): of the neighbour matrix, or of the tunnel block (mapped to nodes through
tunnel_idx + 2); the pair (0, 1) / (1, 0) is the loop_G driver and is left out.  I_rc = (-A_rc) * (m[r] - m[c]), two
rounded operations, exactly what the device does with -ffp-contract=off; the sums here run in CSR order (np.bincount adds
sequentially), the device's in its lanes' order: for a node with n_r pairs and S_r = sum |I_rc| the two differ by at most
n_r * 2**-52 * S_r (two summation orders of the same n_r terms, (n_r - 1) * 2**-53 * S_r each to first order)."""
import math

import numpy as np

EPS = 2.0 ** -52


def pair_list(rp, col, val, row0=0, tunnel=None):
    """(r, c, g, is_tunnel) of the rows row0 ... of a neighbour CSR (global columns) and of a tunnel CSR given as
    dict(tunnel_idx, row_ptr, col, val, first): rows first ... of the block, columns = tunnel point ids."""
    rp, col, val = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float64)
    r = np.repeat(np.arange(len(rp) - 1, dtype=np.int64) + row0, np.diff(rp))
    keep = (col != r) & ~((r < 2) & (col < 2))
    R, Cc, G, Tn = [r[keep]], [col[keep]], [-val[keep]], [np.zeros(int(keep.sum()), bool)]
    if tunnel is not None and len(tunnel["row_ptr"]) > 1:
        trp = np.asarray(tunnel["row_ptr"], np.int64)
        tidx = np.asarray(tunnel["tunnel_idx"], np.int64)
        ti = np.repeat(np.arange(len(trp) - 1, dtype=np.int64) + int(tunnel.get("first", 0)), np.diff(trp))
        tj = np.asarray(tunnel["col"], np.int64)
        k = ti != tj
        R.append(tidx[ti[k]] + 2)
        Cc.append(tidx[tj[k]] + 2)
        G.append(-np.asarray(tunnel["val"], np.float64)[k])
        Tn.append(np.ones(int(k.sum()), bool))
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(G), np.concatenate(Tn)


def node_sums(n_nodes, r, c, g, is_tunnel, m):
    """through, tunnel, net per node + the pair count n and S = sum |I| per node (what the bounds are made of)."""
    m = np.asarray(m, np.float64)
    i_rc = g * (m[r] - m[c])
    a = np.abs(i_rc)
    S = np.bincount(r, a, n_nodes)
    St = np.bincount(r[is_tunnel], a[is_tunnel], n_nodes)
    net = np.bincount(r, i_rc, n_nodes)
    n = np.bincount(r, minlength=n_nodes)
    return dict(G=np.bincount(r, g, n_nodes), through=0.5 * S, tunnel=0.5 * St, net=net, n=n, S=S, St=St, n_t=np.bincount(r[is_tunnel], minlength=n_nodes),
                pairs=len(r), i_rc=i_rc, r=r)


def to_sites(N, atom_site, v):
    """Site array of a node array: zero, then out[atom_site[a]] = v[a + 2] for the atoms with a row (all but the last)."""
    out = np.zeros(N, v.dtype)
    na = len(atom_site) - 1
    out[np.asarray(atom_site)[:na]] = v[2:2 + na]
    return out


def stats(res, atom_site):
    na = len(atom_site) - 1
    th, tu = res["through"][2:2 + na], res["tunnel"][2:2 + na]
    k = int(np.argmax(th)) if na > 0 else -1                      # first maximum = smallest site (atom_site ascends)
    return dict(i_injection=float(res["net"][1]), i_extraction=float(-res["net"][0]), sum_through=math.fsum(th),
                sum_tunnel=math.fsum(tu), max_through=float(th[k]) if na > 0 else 0.0,
                max_site=int(atom_site[k]) if na > 0 else -1, tunnel_pairs_walked=int(res["n_t"].sum()))


def from_parts(n_nodes, rp, col, val, m, row0=0, tunnel=None):
    return node_sums(n_nodes, *pair_list(rp, col, val, row0, tunnel), m)


def from_device(S, buf, m, row0=0):
    """From the device's own exports of ONE rank's rows (solvers.t_pattern / t_vectors / t_tunnel): the neighbour values
    as assembled, the tunnel values as the storage in use holds them."""
    rp, col = S.t_pattern(buf)
    return from_parts(S.t_info(buf)["Nsub"], rp, col, S.t_vectors(buf)["val"], m, row0, S.t_tunnel(buf))


def from_tsystem(T, m):
    """From oracle.TSystem: the neighbour matrix and the tunnel block of the oracle (together merged_csr() minus the
    (0, 1) pair: the two patterns do not overlap off the diagonal, one holds pairs below nn_dist, the other above)."""
    tn = dict(tunnel_idx=T.tunnel_idx, row_ptr=T.sub_row_ptr, col=T.sub_col, val=T.sub_val, first=0) if T.n_t else None
    return from_parts(T.Nsub, T.row_ptr, T.col, T.val, m, 0, tn)
