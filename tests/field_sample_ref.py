"""The restatement kmcf_field_sample and kmcf_field_grid (csrc/kmcf_fieldsample.hip) are held to: the contract of
include/kmcfield.h in plain numpy, and the inputs the tests run it on.  No GPU.

ALL points against ALL members, in blocks of points; the distance written out operation by operation
(site_gap_pbc_ref.d2_exact over the points and the sites in one array: the open difference, or the minimum image through
pbc_ref.c_round, the point first); r2 = radius * radius; u = d2 / r2, t = 1.0 - u, w = t * t; the terms w and w * v are the
bits the library adds.  The restatement adds them with numpy's sum (members in site order); next to it stand the same
sums formed by math.fsum -- the correctly rounded sum, the yardstick of the bounds -- and the sums of w |v|.  No cell
list, no wrap of a point, nothing shared with the kernel.

tests/test_field_sample_ref.py asserts what every input is built for; tests/test_gpu_field_sample.py holds the library to
this file."""
import functools
import math

import numpy as np

import site_gap_pbc_ref as GP

BLOCK = 256                                # points per block of the all-pairs distance
MAX_FIELDS = 8
EPS = 2.0 ** -52
STAT_KEYS = ("n_points", "n_empty", "n_visits", "n_members", "max_count", "max_count_point")
FILL = -7.25


def grid_points(origin, spacing, dims):
    """the points of kmcf_field_grid: origin + index * spacing (a multiplication and an addition), z fastest"""
    o, h = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    i, j, k = np.meshgrid(*(np.arange(int(n), dtype=np.float64) for n in dims), indexing="ij")
    return np.stack([o[0] + i * h[0], o[1] + j * h[1], o[2] + k * h[2]], -1).reshape(-1, 3)


def field_sample(xyz, points, values=None, mask=None, radius=1.0, normalize=1, fill=FILL, L=None):
    """dict(count int32, nearest int32, nearest_d2, wsum, acc (n_fields, n_points): the raw sums, out: what d_out holds,
    wsum_fsum, acc_fsum: the same sums correctly rounded, wabs (n_fields, n_points): the sums of w |v|, stats: the integers of
    kmcf_sample_stats_t); L = (Lx, Ly, Lz): the minimum image, None: open"""
    xyz, points = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(points, np.float64).reshape(-1, 3)
    N, n = len(xyz), len(points)
    values = np.zeros((0, N)) if values is None else np.asarray(values, np.float64).reshape(-1, N)
    nf = len(values)
    mem = np.arange(N) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    both = np.concatenate([points, xyz])
    r2 = np.float64(radius) * np.float64(radius)
    count, nearest = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    nearest_d2 = np.full(n, np.inf)
    wsum, wsum_f = np.zeros(n), np.zeros(n)
    acc, acc_f, wabs = np.zeros((nf, n)), np.zeros((nf, n)), np.zeros((nf, n))
    v_mem = values[:, mem]
    with np.errstate(invalid="ignore"):
        for s0 in range(0, n, BLOCK):
            a = np.arange(s0, min(s0 + BLOCK, n))
            d2 = GP.d2_exact(both, a[:, None], (n + mem)[None, :], L)
            within = d2 <= r2
            u = d2 / r2
            t = 1.0 - u
            w = t * t
            for r, s in enumerate(a):
                sel = np.flatnonzero(within[r])
                count[s] = len(sel)
                if not len(sel):
                    continue
                d = d2[r, sel]
                best = sel[d == d.min()]
                nearest[s], nearest_d2[s] = mem[best].min(), d.min()
                ws = w[r, sel]
                wsum[s], wsum_f[s] = ws.sum(), math.fsum(ws)
                for f in range(nf):
                    term = ws * v_mem[f, sel]
                    acc[f, s] = term.sum()
                    acc_f[f, s] = math.fsum(term) if np.isfinite(term).all() else term.sum()
                    wabs[f, s] = math.fsum(np.abs(term)) if np.isfinite(term).all() else np.inf
        if normalize:
            out = np.where(wsum[None, :] == 0.0, np.float64(fill), acc / np.where(wsum == 0.0, 1.0, wsum)[None, :])
        else:
            out = acc.copy()
    top = int(count.max()) if n else 0
    stats = dict(n_points=n, n_empty=int((count == 0).sum()), n_visits=int(count.astype(np.int64).sum()), n_members=len(mem) if n else 0,
                 max_count=top, max_count_point=int(np.flatnonzero(count == top)[0]) if n else -1)
    return dict(count=count, nearest=nearest, nearest_d2=nearest_d2, wsum=wsum, acc=acc, out=out, wsum_fsum=wsum_f, acc_fsum=acc_f,
                wabs=wabs, stats=stats)


def sample_density(out, radius):
    """the contract of solvers.sample_density, written out once more"""
    return np.asarray(out) * (105.0 / (32.0 * np.pi * float(radius) ** 3))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, L, cutoff = radius of the index, points, values (8, N), mask, radius); the variants of a test (number
# of fields, normalisation, mask, radius, number of points) are applied by reference().

CUTOFF = 6.0
PERIODS = {1: 7.0, 2: 13.0, 3: 19.0, 4: 25.0}                       # cells along an axis of the periodic index: its period
RANDOM = {"r14": (1, 4), "r23": (2, 3), "r32": (3, 2), "r41": (4, 1), "r44": (4, 4)}
TILES = (2047, 2048, 2049)
CELL_COUNTS = (1, 0, 15, 16, 17, 40, 1)                            # sites per index cell along x of the case `cells`
N_POINTS = (0, 1, 15, 16, 17, 257)
FIELD_COUNTS = (0, 1, 2, 3, 4, 5, 8)
SMALL_RADIUS = 1.25
LATTICE_RADIUS = 4.0
ABOVE = 2.0 ** -24                         # (4, ABOVE, 0) from a site: d2 = 16 + 2^-48, the next double above 16


def _values(rng, N):
    """eight rows: normal, the constant 2.5, a 0 / 1 field, then normal rows of growing scale and both signs"""
    v = rng.standard_normal((MAX_FIELDS, N)) * (10.0 ** np.arange(MAX_FIELDS))[:, None]
    v[1] = 2.5
    v[2] = rng.random(N) < 0.3
    return v


def _case(name, xyz, L, cutoff, points, values, mask, radius):
    c = dict(name=name, xyz=np.ascontiguousarray(xyz, np.float64), L=np.array(L, np.float64), cutoff=float(cutoff),
             points=np.ascontiguousarray(points, np.float64), values=np.ascontiguousarray(values, np.float64),
             mask=np.ascontiguousarray(mask, np.int32), radius=float(radius))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _random(name):
    """sites in x in [0, 20), dense towards x = 0, uniform over one period in y and z, the first four pinned to the faces
    of the period; points: 60 % around the sites, 25 % up to 3 periods away in y and z, the rest far out in x (beyond
    reach), and 16 on the faces of the period and their images"""
    ncy, ncz = RANDOM[name]
    Ly, Lz = PERIODS[ncy], PERIODS[ncz]
    rng = np.random.default_rng(7100 + 10 * ncy + ncz)
    N = int(0.09 * 20.0 * Ly * Lz)
    xyz = np.stack([20.0 * rng.random(N) ** 2.5, Ly * rng.random(N), Lz * rng.random(N)], -1)
    xyz[0] = (0.0, 0.0, 0.0)
    xyz[1] = (19.5, np.nextafter(Ly, 0.0), 1.0)
    xyz[2] = (3.0, 1.0, np.nextafter(Lz, 0.0))
    xyz[3] = (20.0, 2.0, 0.0)
    n = 700
    pts = np.stack([-5.0 + 30.0 * rng.random(n), -2.0 + (Ly + 4.0) * rng.random(n), -2.0 + (Lz + 4.0) * rng.random(n)], -1)
    far = rng.random(n)
    k = far < 0.25
    pts[k, 1] = Ly * (-3.0 + 7.0 * rng.random(k.sum()))
    pts[k, 2] = Lz * (-3.0 + 7.0 * rng.random(k.sum()))
    k = far > 0.85
    pts[k, 0] = 27.0 + 30.0 * rng.random(k.sum())
    faces = [(x, y, z) for x in (2.0, 21.5) for y in (0.0, Ly, -Ly, 3.0 * Ly) for z in (0.0, Lz)]
    pts = np.concatenate([pts, np.array(faces)])
    return _case(name, xyz, (20.0, Ly, Lz), CUTOFF, pts, _values(rng, N), rng.random(N) < 0.8, CUTOFF)


def _cells():
    """index cells along x that hold CELL_COUNTS members (every site a member), one cell in y and z"""
    rng = np.random.default_rng(7200)
    xs = []
    for c, m in enumerate(CELL_COUNTS):
        xs.append(6.0 * c + 0.25 + 5.5 * rng.random(m))
    x = np.concatenate(xs)
    N = len(x)
    xyz = np.stack([x, 5.0 * rng.random(N), 5.0 * rng.random(N)], -1)
    xyz[0] = (0.0, 0.0, 0.0)
    n = 400
    pts = np.stack([-3.0 + 48.0 * rng.random(n), -2.0 + 9.0 * rng.random(n), -2.0 + 9.0 * rng.random(n)], -1)
    return _case("cells", xyz, (42.0, 7.0, 7.0), CUTOFF, pts, _values(rng, N), np.ones(N), CUTOFF)


def _tile(n):
    """n sites on a 4 A lattice of 16 x 16 sites per x plane, a mask that keeps about half, 257 points"""
    rng = np.random.default_rng(7300 + n)
    idx = np.arange(n)
    xyz = np.stack([idx // 256, (idx // 16) % 16, idx % 16], -1) * 4.0
    pts = np.stack([-3.0 + 38.0 * rng.random(257), -3.0 + 70.0 * rng.random(257), -3.0 + 70.0 * rng.random(257)], -1)
    return _case("tile@%d" % n, xyz, (36.0, 64.0, 64.0), CUTOFF, pts, _values(rng, n), rng.random(n) < 0.5, CUTOFF)


def _lattice():
    """12 x 16 x 16 sites on the integer lattice in a period of 16 (a power of two: the minimum image is exact), and nine
    lone sites at x = 24; radius 4 on an index of cutoff 4: r2 = 16.  Points on integer and half-integer positions, up to
    more than a period outside in y and z, and nine points at (4, 2^-24, 0) from the lone sites.  Values: small integers.
    Every d2 is a multiple of 1/4 (or 16 + 2^-48), every w a multiple of 1/4096: every sum is exact in any order."""
    rng = np.random.default_rng(7400)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    lone = np.array([(24.0, y, z) for y in (0.0, 5.0, 10.0) for z in (0.0, 5.0, 10.0)])
    xyz = np.concatenate([g, lone])
    N = len(xyz)
    n = 1500
    pts = np.stack([rng.integers(-12, 60, n), rng.integers(-40, 72, n), rng.integers(-40, 72, n)], -1) / 2.0
    pts[:64] = np.floor(pts[:64])                                    # (integer points for certain: on sites, rim at exactly 4)
    pts[64:128, 0] = np.floor(pts[64:128, 0]) + 0.5                  # (ties between two sites)
    pts[64:128, 1:] = np.floor(pts[64:128, 1:])
    pts[:128, 0] = np.clip(pts[:128, 0], 0.0, 11.5)
    above = lone + np.array([4.0, ABOVE, 0.0])
    values = rng.integers(-8, 9, (MAX_FIELDS, N)).astype(np.float64)
    values[1] = 3.0
    mask = rng.random(N) < 0.9
    mask[len(g):] = True                                             # (the lone sites are members)
    return _case("lattice", xyz, (32.0, 16.0, 16.0), LATTICE_RADIUS, np.concatenate([pts, above]), values, mask, LATTICE_RADIUS)


CASES = tuple(RANDOM) + ("cells",) + tuple("tile@%d" % n for n in TILES) + ("lattice",)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in RANDOM:
        return _random(name)
    if name == "cells":
        return _cells()
    if name == "lattice":
        return _lattice()
    return _tile(int(name.split("@")[1]))


def variant(name, n_fields=3, normalize=1, mask="case", radius=None, n_points=None, nan_site=None):
    """the arguments of one call on a case: (points, values or None, mask or None, radius, normalize)"""
    c = case(name)
    pts = c["points"] if n_points is None else c["points"][:n_points]
    values = c["values"][:n_fields] if n_fields else None
    if nan_site is not None:
        values = values.copy()
        values[0, nan_site] = np.nan
    N = len(c["xyz"])
    m = {"case": c["mask"], "null": None, "ones": np.ones(N, np.int32), "none": np.zeros(N, np.int32)}[mask]
    return pts, values, m, c["radius"] if radius is None else float(radius), int(normalize)


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(name, periodic=True, n_fields=3, normalize=1, mask="case", radius=None, n_points=None, nan_site=None):
    """field_sample() of a variant of an input, computed once per process and never modified"""
    c = case(name)
    pts, values, m, r, nrm = variant(name, n_fields, normalize, mask, radius, n_points, nan_site)
    return _freeze(field_sample(c["xyz"], pts, values, m, r, nrm, FILL, c["L"] if periodic else None))
