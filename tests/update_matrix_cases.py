"""Generated cases for the ARS update family (csrc/swimmer_update.hip, csrc/swimmer_update.inc): ars_update_kernel,
ars_update_multi_kernel and ars_update_counted_kernel at both workgroup sizes, and ars_pack_admitted_kernel.  Inputs
and references only: nothing here touches the GPU.  tests/test_update_matrix_cpu.py shows on the references alone that
the cases can catch what they are for, tests/test_update_matrix_gpu.py holds the kernels to them.

THE REFERENCE restates the rule (ars_agent.py:105-130, :179-182; safe_ars/ars.py:41-64), not the kernel:

 * selection: key = max(r+, r-) descending, ties to the higher index; top_b == 0 or top_b >= n_dir uses every direction;
 * sigma = the population standard deviation of the 2k used returns; their mean through math.fsum (exact), the squared
   deviations in np.longdouble, sorted before they are added;
 * step = alpha sum (r+ - r-) delta / (div sigma), div = b when top_b == 0 and the number of used directions otherwise;
   the k products of a policy entry in np.longdouble, added pairwise (np.sum over the contiguous axis): an error of
   ~log2(k) 2^-64 of the absolute sum, 2^-11 of the smallest bound below;
 * V2: the whole list of states ever added, every state with an integer weight (that many copies of it); mean and
   var(ddof = 1) ** -0.5 per column over the list, and the `running` triple {n, mean - c, M2}, c = pi / 2 on the angle
   columns.  The kernel consumes moment rows, so a batch is a few states per row and the rows' sum (x - c), sum
   (x - c)^2 formed from them in long double.

THE BOUNDS are forward-error bounds from the reference's own absolute sums, u = 2^-53, gamma_j = j u / (1 - j u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.4)-(3.5): valid for every order of summation):

 * a sum of k terms followed by a few operations: gamma_(k + 16) sum |terms|;
 * sigma: v = sum (x - mu)^2 has non-negative terms, so gamma_(2k + 16) v; an error e in the computed mu cancels to
   first order (sum (x - mu) = 0) and leaves 2k e^2, e <= gamma_(2k + 16) mean |x|.  sigma = sqrt(v / 2k): half the
   relative error of v, and 4 u for the division and the root;
 * policy: |alpha| / (div sigma) (gamma_(k + 16) A + |g| (rel_sigma + 4 u)) / (1 - rel_sigma - 4 u), A = sum |terms|,
   g = their sum, and u (|policy| + |step|) for the final addition;
 * merge of R rows into `running` (per column, s1 = sum of the rows' sum (x - c), s2 of their squares, S1 and S2 the
   absolute sums, g = gamma_(R + 16), which also pays for the one rounding of each row entry):
     mb = s1 / n_new:            e_mb  = g S1 / n_new
     m2b = s2 - s1 mb:           e_m2b = g (S2 + 2 |mb| S1) + n_new e_mb^2
     mr1 = mr + (mb - mr) n_new / n1 = (n0 mr + n_new mb) / n1:
                                 e_mr1 = (n0 e_mr + n_new e_mb) / n1 + 4 u (|mr| + |mb - mr|)
     m21 = m2 + m2b + (mb - mr)^2 n0 n_new / n1 (non-negative terms):
                                 e_m21 = e_m2 + e_m2b + (n0 n_new / n1) (2 |mb - mr| e + e^2) + 8 u m21, e = e_mb + e_mr
     mean = c + mr1:             e_mean = e_mr1 + u |mean|
     inv_std = (m21 / (n1 - 1)) ** -0.5:   inv_std (r / (2 (1 - r)) + 4 u), r = e_m21 / M2 of the reference
   e_mr and e_m2 are the bounds of the update before (0 at n0 = 0): successive updates on one `running` stay bounded.

A ratio |got - ref| / bound above 1 is a failure, never a reason to widen a bound.  Finite inputs only: NaN returns
are ordered differently by the bitonic path (Python's max, NaN first) and by the ranking paths (fmax) and are left out.
"""
import collections
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
HALF_PI = math.pi / 2                      # kHalfPi (remy_swimmer_env.py:65)
POISON = 1e3                               # in the return slots behind n_dir of a gathered segment
MOM_GROUP = 16                             # kMomGroup: rollouts per moment row
WIDE_FROM, BLOCK, BLOCK_WIDE = 1025, 256, 1024           # kUpdWideFrom, kUpdBlock, kUpdBlockWide
SORT_DIRS, LDS_DIRS = 2048, 6144           # kTopBSortDirs, kUpdMaxDirs
PACK_BLOCK, WAVE = 256, 64                 # kPackBlock, kWave

Ref = collections.namedtuple("Ref", "value bound")       # a reference value (np.longdouble) and its bound (float64)

# the seven kernels of the family: (name, workgroup size of the instantiation or None)
KERNELS = (("ars_update_kernel", 256), ("ars_update_kernel", 1024),
           ("ars_update_multi_kernel", 256), ("ars_update_multi_kernel", 1024),
           ("ars_update_counted_kernel", 256), ("ars_update_counted_kernel", 1024),
           ("ars_pack_admitted_kernel", None))
KERNEL_NAMES = tuple(dict.fromkeys(k for k, _ in KERNELS))


def symbol(name, block):
    """The Itanium spelling of the kernel's own name inside its (anonymous-namespace) symbol."""
    return f"{len(name)}{name}" + (f"ILi{block}EE" if block else "E")


NS = tuple(range(2, 9))
N_DIRS_FULL = (1, 2, 5, 63, 64, 65, 255, 256, 257, 700, 1024, 1025, 1500, 2048, 2049, 6144, 6145)
N_DIRS_EVERY = (5, 257, 1025, 2049)
GATHERED_NS, GATHERED_WORLDS = (2, 3, 6, 8), (1, 2, 3, 8)
GATHERED_N_DIRS = (5, 257, 1025)           # ragged for every world > 1
GATHERED_ALIGNED = (192, 1152)             # chunk a multiple of 8 for every world: the bit-equality claim
MULTI_AGENTS, MULTI_N_DIRS = 3, (9, 1025)
COUNTED_NS, COUNTED_MAX, COUNTED_H = (2, 3, 6, 8), 1030, 3
COUNTS = (0, 5, 1024, 1025, 1030, -3, 2000)              # -3 runs as 0, 2000 as 1030
COUNTED_TOP_B = (0, 700)
PACK_NS, PACK_AGENTS = (2, 8), 3
PACK_N_DIRS = (1, 63, 64, 65, 255, 256, 257, 513, 1030)
PACK_PATTERNS = ("all", "none", "alternating", "random", "last", "wave_heads")


def dims(n):
    """(d, m, m d) of an n-segment swimmer."""
    d = 2 * n + 2
    return d, n - 1, (n - 1) * d


def n_dirs(n):
    return N_DIRS_FULL if n in (2, 8) else N_DIRS_EVERY


def top_bs(n_dir):
    return tuple(dict.fromkeys((0, 1, n_dir // 3, n_dir - 1, n_dir, n_dir + 7)))


def block_of(n_dir):
    return BLOCK_WIDE if n_dir >= WIDE_FROM else BLOCK


def groups(n, block):
    """G: the row groups of the merging workgroup, block // 2d (2d is a power of two at n = 3 and n = 7 only: every
    other n leaves idle threads behind the last group)."""
    return block // (2 * dims(n)[0])


def path(n_dir, top_b):
    """The path of swimmer_update.inc that (n_dir, top_b) takes: (workgroup size, how the used directions are found,
    where the second pass reads its delta column)."""
    select = 0 < top_b < n_dir
    rank = ("none" if not select else "bitonic" if n_dir <= SORT_DIRS else "lds_rank" if n_dir <= LDS_DIRS
            else "global_rank")
    return block_of(n_dir), rank, "registers" if n_dir <= LDS_DIRS else "global"


def merge_path(n, n_dir, rows):
    """(workgroup size, rounds of 8 G rows) of the merging workgroup."""
    return block_of(n_dir), "one_round" if rows <= 8 * groups(n, block_of(n_dir)) else "more_rounds"


def moment_rows(n, block):
    G = groups(n, block)
    return tuple(sorted({1, G - 1, G, G + 1, 8 * G, 8 * G + 1} - {0}))


def rows_of(n_dir):
    """moments_blocks(2 n_dir): the rows that 2 n_dir rollouts write."""
    return (2 * n_dir + MOM_GROUP - 1) // MOM_GROUP


def gamma(j):
    return j * U / (1.0 - j * U)


def ratio(got, ref):
    """max |got - ref.value| / ref.bound over the entries; an entry with bound 0 (a count) must be equal.  A NaN or
    infinite `got` gives inf."""
    got = np.asarray(got, dtype=np.float64)
    diff = np.abs(LD(1) * got - ref.value).astype(np.float64)
    bound = np.broadcast_to(np.asarray(ref.bound, dtype=np.float64), diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    q = np.where(np.isfinite(got), q, np.inf)
    return float(np.max(q))


def _seed(*parts):
    s = 0
    for x in parts:
        s = (s * 1000003 + int(x) + 7) % (2 ** 32)
    return s


# ------------------------------------------------------------------------------------------------------------
# the policy step

@functools.lru_cache(maxsize=None)
def inputs(n, n_dir, agent=0):
    """dict(n, n_dir, returns [2 n_dir], deltas [n_dir, m, d], policy [m, d], alpha, b) of a shape (and agent: unrelated
    data).  The keys max(r+, r-) take few distinct values (many exact ties, and one across every top_b boundary that
    selects); the other return of a direction is 0.1 .. 2 below its key, a different amount for
    every direction, so that no used set has sigma 0.  b is not n_dir."""
    d, m, md = dims(n)
    rs = np.random.RandomState(_seed(n, n_dir, agent))
    levels = np.arange(-3.0, 4.0, 0.5)[:max(1, min(14, (n_dir + 1) // 3))]
    key = np.sort(rs.choice(levels, n_dir))[::-1]
    for tb in top_bs(n_dir):                # a tie across every boundary that selects: the tie rule decides the set
        if 0 < tb < n_dir:
            key[tb] = key[tb - 1]
    key = key[rs.permutation(n_dir)]
    low =key - rs.uniform(0.1, 2.0, n_dir)
    plus = rs.rand(n_dir) < 0.5
    returns = np.empty(2 * n_dir)
    returns[0::2] = np.where(plus, key, low)
    returns[1::2] = np.where(plus, low, key)
    deltas = 2 * rs.rand(n_dir, m, d) - 1
    return dict(n=n, n_dir=n_dir, returns=returns, deltas=deltas, policy=0.3 * (2 * rs.rand(m, d) - 1), alpha=0.02,
                b=float(n_dir + 3))


def select(returns, top_b, ties="higher"):
    """The used directions, ascending.  ties = "lower" is the wrong rule."""
    n_dir = len(returns) // 2
    if top_b <= 0 or top_b >= n_dir:
        return np.arange(n_dir)
    keys = np.maximum(returns[0::2], returns[1::2])
    sign = -1 if ties == "higher" else 1
    order = sorted(range(n_dir), key=lambda i: (-keys[i], sign * i))
    return np.sort(np.array(order[:top_b], dtype=np.int64))


def reference_update(returns, deltas, policy, alpha, b, top_b, ties="higher", ddof=0, divisor="rule"):
    """{"policy": Ref [m, d], "sigma": Ref} of one update.  ties / ddof / divisor other than the defaults are the
    deliberately wrong restatements of tests/test_update_matrix_cpu.py (divisor = "swapped": b where the count is due
    and the count where b is)."""
    returns = np.asarray(returns, dtype=np.float64)
    used = select(returns, top_b, ties)
    k = len(used)
    rp, rm = returns[0::2][used], returns[1::2][used]
    x = np.concatenate([rp, rm])
    mu = LD(math.fsum(x)) / (2 * k)
    sq = np.sort((LD(1) * x - mu) ** 2)
    v = sq.sum()
    sigma = np.sqrt(v / (2 * k - ddof))
    g2k = gamma(2 * k + 16)
    e_mu = g2k * float(np.abs(x).sum()) / (2 * k)
    rel_v = g2k + 2 * k * e_mu ** 2 / float(v)
    rel_sigma = 0.5 * rel_v + 4 * U
    md = policy.size
    terms = (LD(1) * rp - rm)[None, :] * (LD(1) * deltas.reshape(-1, md)[used].T)         # [md, k]
    g, A = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    by_count = (top_b != 0) if divisor == "rule" else (top_b == 0)
    div = LD(k) if by_count else LD(b)
    step = (alpha * g / (div * sigma)).reshape(policy.shape)
    new = LD(1) * policy + step
    scale = abs(alpha) / float(div * sigma)
    e_step = scale * (gamma(k + 16) * A + np.abs(g) * (rel_sigma + 4 * U)) / (1 - rel_sigma - 4 * U)
    e_new = ((1 + U) * e_step.astype(np.float64).reshape(policy.shape)
             + U * (np.abs(policy) + np.abs(step).astype(np.float64)))
    return {"policy": Ref(new, e_new), "sigma": Ref(sigma, float(sigma) * rel_sigma)}


def float64_update(returns, deltas, policy, alpha, b, top_b):
    """The rule in plain float64 with every sum taken sequentially from the LAST term to the first: (policy, sigma).
    The bounds must hold for this too."""
    used = select(returns, top_b)[::-1]
    k = len(used)
    rp, rm = returns[0::2][used], returns[1::2][used]
    x = np.stack([rm, rp], axis=1).ravel()
    mu = np.cumsum(x)[-1] / (2 * k)
    sigma = np.sqrt(np.cumsum((x - mu) ** 2)[-1] / (2 * k))
    g = np.cumsum((rp - rm)[:, None] * deltas.reshape(len(returns) // 2, -1)[used], axis=0)[-1]
    div = float(k) if top_b != 0 else b
    return policy + alpha * (g / (div * sigma)).reshape(policy.shape), sigma


# ------------------------------------------------------------------------------------------------------------
# the V2 statistics

def centre(n):
    c = np.zeros(dims(n)[0])
    c[2::2] = HALF_PI
    return c


def batch(rs, n, weights, shift):
    """One update's states: weights int [rows, s] -> dict(x [rows s, d] float64, w [rows s], rows [rows, 2d] float64:
    what the rollout kernels would leave, n_new).  Column j of the states is c_j + shift_j + N(0, scale_j)."""
    d = dims(n)[0]
    c = centre(n)
    R, s = weights.shape
    x = c + shift + rs.normal(0.0, 1.0, (R, s, d)) * rs.uniform(0.2, 1.0, d)
    y = LD(1) * x - c
    w = (LD(1) * weights)[:, :, None]
    rows = np.concatenate([(w * y).sum(axis=1), (w * y * y).sum(axis=1)], axis=1).astype(np.float64)
    return dict(x=x.reshape(-1, d), w=weights.reshape(-1).astype(np.int64), rows=rows, n_new=int(weights.sum()))


def sequence(n, tag, row_counts, weight_ranges=((1, 10), (5, 21), (1, 10)), weights=None):
    """Successive batches for one `running`: batch u has row_counts[u] rows of three states each, weights from
    weight_ranges[u] (so n_new differs from batch to batch) and its own mean (the batch means move apart).  weights[u]:
    the three weights of every row of batch u in place of drawn ones (agents that share one n_new)."""
    d = dims(n)[0]
    rs = np.random.RandomState(_seed(n, *tag))
    pattern = rs.uniform(0.5, 1.0, d) * rs.choice([-1.0, 1.0], d)
    shifts = (0.0, 0.8, -0.6, 0.4)
    out = []
    for u, R in enumerate(row_counts):
        lo, hi = weight_ranges[u % len(weight_ranges)]
        w = rs.randint(lo, hi, (R, 3)) if weights is None else np.tile(np.asarray(weights[u]), (R, 1))
        out.append(batch(rs, n, w, shifts[u % 4] * pattern))
    return out


def reference_v2(n, batches):
    """After each batch: {"running": Ref [1 + 2d], "mean": Ref [d], "inv_std": Ref [d]} over the list of every state
    added so far; the bounds by the recursion of the module's docstring, from zero at n0 = 0."""
    d = dims(n)[0]
    c = centre(n)
    out = []
    e_mr, e_m2 = np.zeros(d), np.zeros(d)
    mr0, n0 = np.zeros(d, dtype=LD), 0
    xs, ws = [], []
    for bt in batches:
        xs.append(bt["x"])
        ws.append(bt["w"])
        x, w = LD(1) * np.concatenate(xs), (LD(1) * np.concatenate(ws))[:, None]
        n1 = int(np.concatenate(ws).sum())
        mean = np.sort(w * x, axis=0).sum(axis=0) / n1
        M2 = np.sort(w * (x - mean) ** 2, axis=0).sum(axis=0)
        inv_std = (M2 / (n1 - 1)) ** LD(-0.5)
        mr1 = mean - c
        # the bounds, from this batch's rows as the kernel is given them
        rows, n_new = bt["rows"], bt["n_new"]
        g = gamma(rows.shape[0] + 16)
        S1, S2 = np.abs(rows[:, :d]).sum(axis=0), np.abs(rows[:, d:]).sum(axis=0)
        mb = ((LD(1) * rows[:, :d]).sum(axis=0) / n_new).astype(np.float64)
        e_mb = g * S1 / n_new
        e_m2b = g * (S2 + 2 * np.abs(mb) * S1) + n_new * e_mb ** 2
        delta = np.abs(mb - mr0.astype(np.float64))
        e = e_mb + e_mr
        e_mr1 = (n0 * e_mr + n_new * e_mb) / n1 + 4 * U * (np.abs(mr0).astype(np.float64) + delta)
        e_m21 = e_m2 + e_m2b + (n0 * n_new / n1) * (2 * delta * e + e ** 2) + 8 * U * M2.astype(np.float64)
        r = e_m21 / M2.astype(np.float64)
        e_inv = inv_std.astype(np.float64) * (r / (2 * (1 - r)) + 4 * U)
        out.append({"running": Ref(np.concatenate([[LD(n1)], mr1, M2]), np.concatenate([[0.0], e_mr1, e_m21])),
                    "mean": Ref(mean, e_mr1 + U * np.abs(mean).astype(np.float64)),
                    "inv_std": Ref(inv_std, e_inv)})
        e_mr, e_m2, mr0, n0 = e_mr1, e_m21, mr1, n1
    return out


def merge_from_rows(n, batches, drop=None, reverse=False, dtype=LD):
    """The merge restated from the ROWS (Chan et al.), as reference_v2 returns it but without bounds: [(running, mean,
    inv_std)].  drop(u, rows) -> the rows that are summed: the wrong restatements (n_new stays what the rows claimed).
    dtype = np.float64 with reverse = True: the rows added sequentially from the last to the first in plain float64."""
    d = dims(n)[0]
    c = centre(n).astype(dtype)
    n0, mr, m2 = 0, np.zeros(d, dtype=dtype), np.zeros(d, dtype=dtype)
    out = []
    for u, bt in enumerate(batches):
        rows = bt["rows"] if drop is None else drop(u, bt["rows"])
        rows = rows.astype(dtype)[::-1] if reverse else rows.astype(dtype)
        s = np.cumsum(rows, axis=0)[-1] if len(rows) else np.zeros(2 * d, dtype=dtype)
        n_new = bt["n_new"]
        n1 = n0 + n_new
        mb = s[:d] / n_new
        m2b = s[d:] - s[:d] * mb
        delta = mb - mr
        mr = mr + delta * (dtype(n_new) / n1)
        m2 = (m2 + m2b) + delta * delta * (dtype(n0) * n_new / n1)
        n0 = n1
        out.append((np.concatenate([[dtype(n1)], mr, m2]), c + mr, (m2 / (n1 - 1)) ** dtype(-0.5)))
    return out


@functools.lru_cache(maxsize=None)
def moment_case(n, n_dir, rows):
    """Three successive updates with `rows` moment rows each (passed independently of n_dir): (batches, references)."""
    batches = sequence(n, (n_dir, rows, 1), (rows,) * 3)
    return batches, reference_v2(n, batches)


def moment_top_bs(n_dir):
    """top_b of the three updates of a moment case."""
    return 0, n_dir // 3, n_dir - 1


# ------------------------------------------------------------------------------------------------------------
# the gathered layout (world > 1): `world` segments [2 chunk returns | rows_chunk moment rows of 2d]

def shard_rows(n_dir, world):
    """(chunk, rows_chunk, the real rows of every rank): chunk = ceil(n_dir / world); a rank's rollouts fill
    ceil(2 count / 16) rows of its rows_chunk, the rest stay zero as the host leaves them."""
    chunk = -(-n_dir // world)
    counts = [min(chunk, max(0, n_dir - r * chunk)) for r in range(world)]
    return chunk, rows_of(chunk), [rows_of(c) for c in counts]


def row_aligned(n_dir, world):
    return n_dir % world == 0 and (n_dir // world) % 8 == 0


@functools.lru_cache(maxsize=None)
def gathered_case(n, n_dir, world):
    """Two successive updates in the gathered layout: dict(chunk, rows_chunk, buffers: the two gathered arrays,
    batches, flat_rows: the real rows of each update in global order, refs_v2).  The returns are inputs(n, n_dir)'s.
    With row-aligned shards the real rows are the same for every world, world = 1 included."""
    d = dims(n)[0]
    chunk, rows_chunk, real = shard_rows(n_dir, world)
    batches = sequence(n, (n_dir, 2), (sum(real),) * 2)
    returns = inputs(n, n_dir)["returns"]
    seg = 2 * chunk + rows_chunk * 2 * d
    buffers = []
    for bt in batches:
        buf = np.zeros((world, seg))
        at = 0
        for r in range(world):
            lo, hi = min(n_dir, r * chunk), min(n_dir, (r + 1) * chunk)
            buf[r, :2 * chunk] = POISON
            buf[r, :2 * (hi - lo)] = returns[2 * lo:2 * hi]
            buf[r, 2 * chunk:2 * chunk + real[r] * 2 * d] = bt["rows"][at:at + real[r]].ravel()
            at += real[r]
        buffers.append(buf.ravel())
    return dict(chunk=chunk, rows_chunk=rows_chunk, buffers=buffers, batches=batches, refs_v2=reference_v2(n, batches))


def gathered_returns(buf, n, n_dir, world, chunk, rows_chunk, index_chunk=None):
    """The returns [2 n_dir] as the layout holds them.  index_chunk: the chunk that direction -> (rank, slot) is
    computed with (the wrong restatement: n_dir // world); a rank beyond the world reads POISON."""
    seg = 2 * chunk + rows_chunk * 2 * dims(n)[0]
    ic = chunk if index_chunk is None else index_chunk
    out = np.full(2 * n_dir, POISON)
    for i in range(n_dir):
        rank, local = divmod(i, ic)
        if rank < world:
            out[2 * i:2 * i + 2] = buf[rank * seg + 2 * local:rank * seg + 2 * local + 2]
    return out


# ------------------------------------------------------------------------------------------------------------
# multi and counted: S agents with unrelated data

@functools.lru_cache(maxsize=None)
def multi_case(n, n_dir):
    """S = 3 agents: dict(agents: inputs(n, n_dir, a), batches[a]: two successive batches of rows_of(n_dir) rows,
    refs_v2[a]); top_b = n_dir // 3.  A launch has one n_new_states: the agents' rows carry the same weights."""
    agents = [inputs(n, n_dir, a) for a in range(MULTI_AGENTS)]
    batches = [sequence(n, (n_dir, 3, a), (rows_of(n_dir),) * 2, weights=((4, 3, 9), (6, 7, 5)))
               for a in range(MULTI_AGENTS)]
    return dict(agents=agents, batches=batches, refs_v2=[reference_v2(n, b) for b in batches], top_b=n_dir // 3)


@functools.lru_cache(maxsize=None)
def counted_case(n):
    """len(COUNTS) agents of COUNTED_MAX directions: dict(returns [S, 2N], deltas [S, N, m, d], policy [S, m, d],
    moments [S, rows_of(N), 2d], running [S, 1 + 2d]: a state in mid-training (n0 > 0), alpha, b)."""
    d = dims(n)[0]
    S = len(COUNTS)
    agents = [inputs(n, COUNTED_MAX, 10 + a) for a in range(S)]
    rs = np.random.RandomState(_seed(n, 4))
    moments = np.stack([batch(rs, n, np.full((rows_of(COUNTED_MAX), 3), [7, 5, 4]) * COUNTED_H,
                              rs.uniform(-0.5, 0.5, d))["rows"] for _ in range(S)])
    running = np.concatenate([rs.randint(40, 90, (S, 1)).astype(np.float64), rs.uniform(-0.3, 0.3, (S, d)),
                              rs.uniform(5.0, 20.0, (S, d))], axis=1)
    return dict(returns=np.stack([a["returns"] for a in agents]), deltas=np.stack([a["deltas"] for a in agents]),
                policy=np.stack([a["policy"] for a in agents]), moments=moments, running=running, alpha=0.02,
                b=float(COUNTED_MAX + 3))


def counted_n_dir(count):
    return min(max(count, 0), COUNTED_MAX)


# ------------------------------------------------------------------------------------------------------------
# pack

def pattern(name, n_dir, rs):
    """admit flags int32 [n_dir]: non-zero values of either sign mean admitted."""
    i = np.arange(n_dir)
    on = {"all": np.ones(n_dir, bool), "none": np.zeros(n_dir, bool), "alternating": i % 2 == 1,
          "random": rs.rand(n_dir) < 0.5, "last": i == n_dir - 1, "wave_heads": i % WAVE == 0}[name]
    return np.where(on, rs.choice([1, -1, 7], n_dir), 0).astype(np.int32)


@functools.lru_cache(maxsize=None)
def pack_case(n, n_dir, name, with_status):
    """dict(admit int32 [S, N], status int32 [S, 2N] or None, deltas [S, N, m, d]).  Agent 0 has the named pattern,
    agent 1 a random one, agent 2 the next pattern of the list; the status refuses a few directions on the + or on
    the - rollout."""
    d, m, _ = dims(n)
    rs = np.random.RandomState(_seed(n, n_dir, PACK_PATTERNS.index(name), with_status, 5))
    names = (name, "random", PACK_PATTERNS[(PACK_PATTERNS.index(name) + 1) % len(PACK_PATTERNS)])
    admit = np.stack([pattern(k, n_dir, rs) for k in names])
    status = None
    if with_status:
        status = np.zeros((PACK_AGENTS, 2 * n_dir), dtype=np.int32)
        for a in range(PACK_AGENTS):
            hit = rs.choice(2 * n_dir, max(1, n_dir // 6), replace=False)
            status[a, hit] = rs.choice([3, -2], len(hit))
    return dict(admit=admit, status=status, deltas=2 * rs.rand(PACK_AGENTS, n_dir, m, d) - 1)


def reference_pack(admit, status, deltas, restart=None):
    """(count [S], order [S, N] padded with -1, packed [S, N, m, d] with NaN where nothing is written).  restart = 64 or
    256: the wrong restatement whose positions restart at each wave or round (later writes win, as in memory)."""
    S, N = admit.shape
    on = admit != 0
    if status is not None:
        on = on & (status[:, 0::2] == 0) & (status[:, 1::2] == 0)
    count = on.sum(axis=1).astype(np.int32)
    order = np.full((S, N), -1, dtype=np.int32)
    packed = np.full(deltas.shape, np.nan)
    for a in range(S):
        idx = np.flatnonzero(on[a])
        if restart is None:
            order[a, :len(idx)] = idx
        else:
            for i in idx:
                order[a, int(on[a, i - i % restart:i].sum())] = i
        for j in range(count[a]):
            if order[a, j] >= 0:
                packed[a, j] = deltas[a, order[a, j]]
    return count, order, packed
