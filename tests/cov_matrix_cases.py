"""Cases, reference, tiling and bound for the covariance family (csrc/swimmer_cov.h, csrc/swimmer_cov.hip): the
standalone pass traj_moments_kernel<D, BLOCK> behind sw_traj_moments_f64, the passes an ARS pipeline launch leaves owed
(flushed by launch_traj_moments with the owed block, or run by side_cov_tile<D, BLOCK> workgroups inside the next
rollout launch), and the host arithmetic of cov_tiling / sw_cov_acc_doubles.  No GPU here:
tests/test_cov_matrix_cpu.py checks on this file alone that the cases reach what tests/test_cov_matrix_gpu.py is there
for, and that the bound would show the mistakes it is there for.

REFERENCE (reference).  A trajectory s [H, d, R] in float64.  x = fl64(s - c) with c the pi / 2 double on the even
columns >= 2 (kHalfPi): one correctly rounded subtraction, the kernel's own first operation, so both sides start from
the same x.  Then S1_f = sum x_f and S2_fg = sum x_f x_g over all steps and rollouts in np.longdouble (64-bit
significand), summed by a halving tree: at most ceil(log2 N) + 1 roundings of 2^-64 per path (REF_SLACK covers them
for N < 2^30).  With them the condition sums A1_f = sum |x_f| and A2_fg = sum |x_f x_g|.

BOUND (additions, bound).  Every product x_f x_g is formed inside an fma (moments_pass, moments_item_add), so only
the additions round, one rounding per fma or add; the first-moment sums are plain adds.  A sum that reaches acc over a
path of L roundings is off by at most ((1 + u)^L - 1) A, u = 2^-53.  L is read off csrc/swimmer_cov.h:
   tchunk   sequential fma / add in a lane, one per step of the tile (moments_pass's t loop; the split form's
            add(xa) .. add(xc), which keep the steps in order)
   6        __shfl_down levels over the 64 lanes (off = 32 .. 1), both forms
   BLOCK/64 the wave partials added in LDS order, WIDE form only (moments_pass: v += sh[i * W + j]); the split form
            stores each wave's own items, no cross-wave sum
   ceil(n_tiles / 256)   the merge: lane l adds tiles l + 64 i + 256 k into partial a[e][i] (main loop and 3-step tail)
   2        (a0 + a1) + (a2 + a3)
   6        __shfl_down levels of the merge
   1        acc[...] += v
and one more for every earlier pass into the same acc (or a pre-filled acc).  Some of these add to an exact zero and
do not round; the bound counts them all the same.  The count entry and S2 == S2.T are exact.  The bound is never
measured on a kernel; what a GPU run observed, |got - ref| / (u A) per kernel form, is a record
(profiles/cov_matrix_observed.json).

DATA (data).  Three regimes, seeded per case:
   a  |x| uniform in [0.5, 2] with random signs: every term is >= 0.25 while the sums cancel -- only a bound
      relative to A means anything there
   b  large offsets, small spread: positions near +-1e3, angles pi / 2 + 2 pi k + noise, angular velocities near +-50:
      the regime in which S2 - S1 S1^T / n cancels on the host
   c  index-coded: x[t, j, r] = K 2^-10 with K an integer in -438 .. 438 made of (t, j, r).  s = c + K 2^-10 is exact
      (c lies in [1, 2) with ulp 2^-52, and so does s), hence x is, every product is an integer times 2^-20, and every
      partial sum stays below 2^53 of those units: the kernel must be BIT-EXACT, in whatever order it adds.  A swapped
      column, a transposed store, a skipped or doubled step or a lane that reads r >= R changes an integer.
"""
import collections
import math
import os
import zlib

import numpy as np

from swimmer_amd import _lib

U = 2.0 ** -53
REF_SLACK = 2.0 ** -59            # 32 roundings of 2^-64: the reference's own halving tree and its leaf products
HALF_PI = math.pi / 2             # kHalfPi
WAVE = 64
MOM_BLOCK = 256                   # kMomBlock: the standalone pass
MOM_TCHUNK = 32                   # kMomTChunk
MAX_TILES = 4096                  # kCovMaxTiles
OWED_BLOCKS = (128, 64, 256, 256)  # owed_cov_block of the forms Oct3, Quad3, Row, Lane (sw_cov_acc_doubles' loop)
NS = tuple(range(2, 9))
KNOBS = ("SWIMMER_COV_TCHUNK", "SWIMMER_COV_NAP")


def knobs_set():
    """The measurement knobs that change the tiling (or the pacing) under test; read once per process by the library."""
    return [k for k in KNOBS if os.environ.get(k) is not None]


def dims(n):
    return 2 * n + 2


def cov_sums(D):
    return 1 + D + D * D


def cov_split(D, block):
    return D >= 12 and block >= 256


def form_name(D, block):
    """The tile form of an instantiation, as the test ids and the observed record name it."""
    return "D%d_B%d_%s" % (D, block, "split" if cov_split(D, block) else "wide")


# ------------------------------------------------------------------------------------------------ tiling
Tiling = collections.namedtuple("Tiling", "cols nbx ny tchunk lengths n_tiles")


def tiling(n_roll, H, block, D, riding):
    """cov_tiling (csrc/swimmer_cov.hip) restated, without the SWIMMER_COV_TCHUNK knob."""
    split = cov_split(D, block)
    cols = WAVE if split else block
    nbx = (n_roll + cols - 1) // cols
    base = (4 * MOM_TCHUNK if split else MOM_TCHUNK) if block >= MOM_BLOCK else 128
    if not riding:
        target = 256 if split else 128
        want = (H * nbx + target - 1) // target
        base = 8 if want < 8 else (H if want > H else want)
    ny_max = (H + base - 1) // base
    cap = max(MAX_TILES // nbx, 1)
    ny = min(ny_max, cap)
    tchunk = (H + ny - 1) // ny
    ny = (H + tchunk - 1) // tchunk
    lengths = tuple(min(H, (by + 1) * tchunk) - by * tchunk for by in range(ny))
    return Tiling(cols, nbx, ny, tchunk, lengths, nbx * ny)


def acc_doubles(n, n_roll, H, blocks=OWED_BLOCKS):
    """sw_cov_acc_doubles restated: the sums, the ticket and one row per tile of the largest pass the batch can get."""
    D = dims(n)
    tiles = 0
    if n_roll > 0 and H > 0:
        tiles = max(tiling(n_roll, H, b, D, riding).n_tiles for riding in (False, True) for b in blocks)
    return cov_sums(D) + 1 + tiles * (D + D * D)


def split_tail(length):
    """moments_split_wave's control for a tile of `length` steps: (trips of the three-step loop, left)."""
    t = trips = 0
    while t + 4 < length:
        t += 3
        trips += 1
    return trips, length - t


def split_items(D):
    """(ITEMS, PER) of the split form: wave w owns items [w PER, (w + 1) PER)."""
    items = D + D * (D + 1) // 2
    return items, (items + 3) // 4


def item_entry(D, q):
    """Item q of a tile's sums -> ('s1', j) or ('s2', f, g): first moments, then the upper triangle row-major."""
    if q < D:
        return ("s1", q)
    p, f = q - D, 0
    while p >= D - f:
        p -= D - f
        f += 1
    return ("s2", f, f + p)


# ------------------------------------------------------------------------------------------------ bound
def additions(t, block, D, earlier_passes=0):
    """Roundings on the longest path from a leaf to acc (the table in the module docstring)."""
    wide = 0 if cov_split(D, block) else block // WAVE
    return t.tchunk + 6 + wide + (t.n_tiles + 255) // 256 + 2 + 6 + 1 + earlier_passes


def gamma(L):
    return (np.longdouble(1) + np.longdouble(U)) ** L - np.longdouble(1) + np.longdouble(REF_SLACK)


Ref = collections.namedtuple("Ref", "count S1 S2 A1 A2")


def bounds(ref, L):
    g = gamma(L)
    return g * ref.A1, g * ref.A2


def ratios(got, ref):
    """(worst |got - ref| / (u A) over S1, over S2) of an accumulator's sums: the observed record."""
    D = ref.S1.shape[0]
    s1, s2 = unpack(got, D)[1:]
    e1 = np.abs(s1.astype(np.longdouble) - ref.S1) / (np.longdouble(U) * ref.A1)
    e2 = np.abs(s2.astype(np.longdouble) - ref.S2) / (np.longdouble(U) * ref.A2)
    return float(e1.max()), float(e2.max())


def unpack(acc, D):
    acc = np.asarray(acc)
    return acc[0], acc[1:1 + D], acc[1 + D:1 + D + D * D].reshape(D, D)


def violations(got, ref, L):
    """What is wrong with the sums `got` (count | S1 | S2 as the kernel lays them out): a list, empty when the count
    is exact, S2 is symmetric bit for bit, and every entry is inside its bound."""
    D = ref.S1.shape[0]
    count, s1, s2 = unpack(got, D)
    b1, b2 = bounds(ref, L)
    out = []
    if count != ref.count:
        out.append(("count", float(count), float(ref.count)))
    if not np.array_equal(s2, s2.T):
        out.append(("symmetry", np.argwhere(s2 != s2.T)[:4].tolist()))
    e1 = np.abs(s1.astype(np.longdouble) - ref.S1)
    e2 = np.abs(s2.astype(np.longdouble) - ref.S2)
    if not (e1 <= b1).all():
        j = int(np.argmax(e1 - b1))
        out.append(("S1", j, float(e1[j]), float(b1[j])))
    if not (e2 <= b2).all():
        f, g = np.unravel_index(int(np.argmax(e2 - b2)), e2.shape)
        out.append(("S2", int(f), int(g), float(e2[f, g]), float(b2[f, g])))
    return out


def tile_partials(traj, t):
    """What every tile of the tiling t sums into S2[0, 0], in tile order (tile = by nbx + bx): exact in regime c,
    where it pins the tiling a pass really took -- columns per tile, steps per tile and the order of the tiles."""
    x = centred(traj)
    H, _, R = x.shape
    sq = np.zeros((t.ny * t.tchunk, t.nbx * t.cols))
    sq[:H, :R] = x[:, 0, :] ** 2
    return sq.reshape(t.ny, t.tchunk, t.nbx, t.cols).sum(axis=(1, 3)).ravel()


def packed(ref):
    """The reference rounded to float64 in the accumulator's layout (exact in regime c)."""
    return np.concatenate(([ref.count], ref.S1.astype(np.float64), ref.S2.astype(np.float64).ravel()))


# ------------------------------------------------------------------------------------------------ reference
def pivots(D):
    c = np.zeros(D)
    c[2::2] = HALF_PI
    return c


def centred(traj):
    """x = fl64(s - c): the one float64 operation the reference shares with the kernel."""
    traj = np.asarray(traj, dtype=np.float64)
    return traj - pivots(traj.shape[1])[None, :, None]


def _tree(v):
    """Sums over the last axis by halving: at most ceil(log2 N) roundings on any path."""
    v = np.asarray(v, dtype=np.longdouble)
    while v.shape[-1] > 1:
        if v.shape[-1] & 1:
            v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), np.longdouble)], axis=-1)
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def reference_of_x(x):
    """The long-double sums of centred data x [H, D, R]."""
    H, D, R = x.shape
    xl = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(D, H * R)).astype(np.longdouble)
    S1, A1 = _tree(xl), _tree(np.abs(xl))
    S2 = np.zeros((D, D), np.longdouble)
    A2 = np.zeros((D, D), np.longdouble)
    for f in range(D):
        prod = xl[f][None, :] * xl[f:]
        S2[f, f:] = S2[f:, f] = _tree(prod)
        A2[f, f:] = A2[f:, f] = _tree(np.abs(prod))
    return Ref(np.longdouble(H) * R, S1, S2, A1, A2)


def reference(traj):
    return reference_of_x(centred(traj))


def reference_exact(traj):
    """The same for regime c, where every sum is an integer multiple of 2^-20 below 2^53 of them: float64 matrix
    products are exact there, in any order (tests/test_cov_matrix_cpu.py holds it against reference())."""
    x = centred(traj)
    H, D, R = x.shape
    k = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(D, H * R)) * 1024.0
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= C_MAX
    a = np.abs(k)
    A2 = a @ a.T
    assert A2.max() < 2.0 ** 52
    ld = np.longdouble
    return Ref(ld(H) * R, k.sum(axis=1).astype(ld) / 1024, (k @ k.T).astype(ld) / 1024 ** 2,
               a.sum(axis=1).astype(ld) / 1024, A2.astype(ld) / 1024 ** 2)


# ------------------------------------------------------------------------------------------------ data
REGIMES = ("a", "b", "c")
C_MAX = 438


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def index_code(H, D, R):
    """K[t, j, r]: an integer in -438 .. 438 made of the three indices (877 is prime)."""
    t = np.arange(H, dtype=np.int64)[:, None, None]
    j = np.arange(D, dtype=np.int64)[None, :, None]
    r = np.arange(R, dtype=np.int64)[None, None, :]
    return (191 * t + 313 * j + 17 * r + 29 * ((t * (j + 1) * (r + 3)) % 11)) % 877 - C_MAX


def data(regime, n, H, R):
    """A trajectory [H, d, R] of the regime, seeded by (regime, n, H, R)."""
    D = dims(n)
    c = pivots(D)[None, :, None]
    rs = _rs("cov", regime, n, H, R)
    if regime == "a":
        x = rs.uniform(0.5, 2.0, (H, D, R)) * rs.choice((-1.0, 1.0), (H, D, R))
        return x + c
    if regime == "b":
        s = np.empty((H, D, R))
        s[:, 0] = 1e3 + 1e-3 * rs.standard_normal((H, R))
        s[:, 1] = -1e3 + 1e-3 * rs.standard_normal((H, R))
        for j in range(2, D):
            if j % 2 == 0:     # an angle that has wound k times
                s[:, j] = HALF_PI + 2 * math.pi * ((j // 2) % 7 - 3) + 1e-2 * rs.standard_normal((H, R))
            else:
                s[:, j] = 50.0 * (-1) ** (j // 2) + 1e-2 * rs.standard_normal((H, R))
        return s
    assert regime == "c"
    s = c + index_code(H, D, R) / 1024.0
    assert np.array_equal((s - c) * 1024.0, index_code(H, D, R))
    return s


def reference_for(regime, traj):
    return reference_exact(traj) if regime == "c" else reference(traj)


# ------------------------------------------------------------------------------------------------ standalone cases
STANDALONE_H = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13)
R_SPLIT = (1, 63, 64, 65)
R_WIDE = R_SPLIT + (255, 256, 257)


def standalone_shapes(n):
    """(R, H) of the standalone pass of traj_moments_kernel<2 n + 2, 256>."""
    rs = R_SPLIT if cov_split(dims(n), MOM_BLOCK) else R_WIDE
    return tuple((R, H) for R in rs for H in STANDALONE_H)


# The merge at n_tiles 1, 2, 63..65, 127..129, 191..193, 255..257 and beyond 320: (n, R, H), chosen with tiling();
# every class at n = 3 (wide, 256 columns) and at n = 6 (split, 64 columns), ragged last tiles along both axes.
MERGE_CASES = (
    (3, 200, 7), (3, 200, 9), (3, 300, 9), (3, 16000, 5), (3, 513, 161), (3, 16384, 3), (3, 16385, 2), (3, 1025, 97),
    (3, 32257, 1), (3, 4096, 64), (3, 32769, 3), (3, 10753, 17), (3, 48641, 2), (3, 24321, 9), (3, 49153, 2), (3, 25089, 9),
    (3, 65025, 1), (3, 65536, 2), (3, 65537, 1), (3, 82177, 2), (3, 3300, 89), (3, 3500, 98), (3, 3500, 116),
    (6, 60, 8), (6, 100, 5), (6, 4031, 3), (6, 1024, 32), (6, 4097, 2), (6, 8127, 2), (6, 2048, 29), (6, 8193, 1),
    (6, 12223, 2), (6, 768, 128), (6, 12289, 1), (6, 1087, 120), (6, 16384, 2), (6, 16385, 1), (6, 832, 160),
    (6, 832, 208), (6, 832, 246), (6, 10497, 9),
)
N_TILES_CLASSES = ((1, 1), (2, 2), (63, 65), (127, 129), (191, 193), (255, 257), (321, MAX_TILES))
# the cap of 4096 tiles binding on nbx: 4097 column tiles of 64 rollouts, ny = 1 (about 50 MB)
CAP_CASE = (5, 262145, 2)
# two passes of different shapes into one acc sized for the larger: (n, (R, H) first, (R, H) second)
TWO_SHAPE_CASES = ((3, (300, 9), (4095, 136)), (3, (4095, 136), (65, 3)), (6, (832, 160), (65, 5)),
                   (6, (100, 5), (1087, 120)))

# ------------------------------------------------------------------------------------------------ owed passes
RidingForm = collections.namedtuple("RidingForm", "name n flags quad_env block rides")
RIDING_FORMS = (
    RidingForm("oct3", 3, 0, False, 128, True),
    RidingForm("quad3", 3, 0, True, 64, True),
    RidingForm("row", 4, 0, False, 256, True),
    RidingForm("row", 5, 0, False, 256, True),
    RidingForm("row", 6, 0, False, 256, True),
    RidingForm("row", 7, 0, False, 256, True),
    RidingForm("row", 8, 0, False, 256, True),
    RidingForm("lane", 2, 0, False, 256, False),
    RidingForm("lane", 6, _lib.FLAG_ROLLOUT_LANE, False, 256, False),
)


def riding_id(f):
    """The kernels an owed pass of the form runs in: side_cov_tile<D, BLOCK> inside the next rollout launch, and
    traj_moments_kernel<D, BLOCK> with the riding tiling when it is flushed (the lane form: the flush only)."""
    D = dims(f.n)
    ride = "side_cov_tile_%s-" % form_name(D, f.block) if f.rides else ""
    return "%s_n%d-%sflush_traj_moments_kernel_%s" % (f.name, f.n, ride, form_name(D, f.block))


N_DIRS = (1, 32, 33, 65, 129)            # 2, 64, 66, 130 and 258 rollouts
EXTRA_N_DIRS = (31, 63, 127)             # 62, 126, 254: the last column tile two lanes short (rollouts come in pairs)


def riding_T(f):
    """Steps per tile of the form's riding tiling where the cap does not bind: 128, or 32 for the wide 256-thread tiles."""
    return tiling(2, 1024, f.block, dims(f.n), True).tchunk


def riding_shapes(f):
    """(n_dir, H): every n_dir at H = 5 and T + 1, every H at 33 and 129 directions, T the form's riding tchunk."""
    T = riding_T(f)
    hs = (1, 2, 5, T - 1, T, T + 1, 2 * T + 3)
    out = [(nd, h) for nd in N_DIRS for h in (5, T + 1)]
    out += [(nd, h) for h in hs for nd in (33, 129) if (nd, h) not in out]
    out += [(nd, 5) for nd in EXTRA_N_DIRS]
    return tuple(out)


# one pass per form with more than 192 tiles (the fourth interleaved partial of the merge in the form's own
# instantiation): (n_dir, H), every regime.  The mirror-quad and the split row shapes are two column tiles wide and 97
# step tiles long, which keeps their buffers near 100 MB.
BIG_RIDING = {
    ("oct3", 3): (65, 12289),           # 2 x 97 = 194 tiles of 128 x 127, 102 MB
    ("quad3", 3): (1056, 769),          # 33 x 7 = 231 tiles of 64 x 110, 104 MB
    ("row", 4): (385, 1537),            # 4 x 49 = 196 tiles of 256 x 32, 95 MB
    ("row", 5): (33, 12289),            # 2 x 97 = 194 tiles of 64 x 127, 78 MB
    ("lane", 2): (385, 1537),           # flushed with 256 threads: 4 x 49 = 196 tiles of 256 x 32, 57 MB
}
# the quad kernel where plan_rollouts picks it by itself: more than 8192 rollouts
QUAD_NATURAL = (4097, 5)


Pass = collections.namedtuple("Pass", "where n D block riding R H")


def gpu_passes():
    """Every covariance pass of tests/test_cov_matrix_gpu.py, for the coverage asserts of the CPU file."""
    out = []
    for n in NS:
        for R, H in standalone_shapes(n):
            out.append(Pass("standalone", n, dims(n), MOM_BLOCK, False, R, H))
    for n, R, H in MERGE_CASES + (CAP_CASE,):
        out.append(Pass("merge", n, dims(n), MOM_BLOCK, False, R, H))
    for f in RIDING_FORMS:
        shapes = list(riding_shapes(f))
        if (f.name, f.n) in BIG_RIDING:
            shapes.append(BIG_RIDING[(f.name, f.n)])
        if f.name == "quad3":
            shapes.append(QUAD_NATURAL)
        for n_dir, H in shapes:
            out.append(Pass("owed", f.n, dims(f.n), f.block, True, 2 * n_dir, H))
    return out


# ------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("step_dropped", "step_doubled", "pivot_kept", "not_mirrored", "wave_boundary_item", "count_one_tile")


def mutate(kind, traj, ref, t, D):
    """The sums a kernel with one mistake would deliver, from the reference: acc layout, float64.  t: the tiling."""
    x = centred(traj).astype(np.longdouble)
    count, S1, S2 = ref.count, ref.S1.copy(), ref.S2.copy()
    cols = slice(0, min(t.cols, x.shape[2]))             # the first column tile, step 0 of the first step tile
    if kind in ("step_dropped", "step_doubled"):
        sign = -1 if kind == "step_dropped" else 1
        xs = x[0, :, cols]
        S1 += sign * xs.sum(axis=1)
        S2 += sign * (xs @ xs.T)
    elif kind == "pivot_kept":
        j = 2
        raw = np.asarray(traj, dtype=np.float64).astype(np.longdouble)[:, j, :]
        S1[j] = raw.sum()
        for g in range(D):
            v = (raw * (raw if g == j else x[:, g, :])).sum()
            S2[j, g] = S2[g, j] = v
    elif kind == "not_mirrored":
        S2[D - 1, 1] = 0
    elif kind == "wave_boundary_item":
        _, per = split_items(D)
        a, b = item_entry(D, per), item_entry(D, per - 1)      # item Q0 of wave 1 lands where its neighbour belongs

        def get(e):
            return S1[e[1]] if e[0] == "s1" else S2[e[1], e[2]]

        def put(e, v):
            if e[0] == "s1":
                S1[e[1]] = v
            else:
                S2[e[1], e[2]] = S2[e[2], e[1]] = v
        va, vb = get(a), get(b)
        put(a, vb)
        put(b, va)
    elif kind == "count_one_tile":
        count = count - (cols.stop - cols.start) * t.lengths[0]
    else:
        raise ValueError(kind)
    return np.concatenate(([count], S1.astype(np.float64), S2.astype(np.float64).ravel()))
