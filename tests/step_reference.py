"""A long-double reference for the step family (csrc/swimmer_step.hip), and the bounds the kernels are held to.
Nothing here touches the GPU.

THE REFERENCE restates the two models statement by statement in np.longdouble (64-bit significand), vectorised over
environments, not the kernels' reduced n x n algebra:

 * Gym model: compute_accelerations as oracle/swimmer_oracle.c:78-174 states it (points' speeds and affine
   accelerations, change of frame, joint forces, the (n + 2) x (n + 3) dynamic matrix), solved by elimination with
   partial pivoting; explicit Euler and reward = Gdot_new . direction (:176-196).
 * Twin model: oracle/twin_oracle.c: compute_friction (:61-92), the dense (5n + 2) system (:94-143) assembled and
   solved in long double, Gdd the mean of the Gdd_i (:156-161), semi-implicit Euler (:185-203).

Sines and cosines are INPUTS of the acceleration functions, so that the condition term can perturb them; the step
functions form them from the angles taken as exact doubles.

THE BOUNDS.  u = 2^-53, gamma_j = j u / (1 - j u) (Higham, Accuracy and Stability of Numerical Algorithms, (3.4)).

 * accelerations, per ENVIRONMENT (normwise; a per-output bound is useless next to thdd ~ 1e5):
       bound = K u max_j (C_j + |ref_j|),    C_j = sum_x |d f_j / d x| w_x
   by central differences of the long-double function with step 2^-26; x ranges over the sines and cosines (w = 1:
   an ABSOLUTE perturbation by one unit, the in-kernel polynomial has an absolute error of ~2.3e-16 wherever the
   angle is, tests/test_trig_range.py), and thetadot, Gdot, u, l, m, k (w = |x|: relative).  K is measured on the
   fp64 ORACLE, never on a kernel (tests/test_step_matrix_cpu.py): K = 4 R_oracle rounded up to a power of two.
 * step: thd' = thd + h a: h bound_a + 2 u (|thd| + |h a|); Gdot likewise; th' = th + h thd (Gym: the old thd):
   2 u (|th| + |h thd|), and for the twin's th' = th + h thd' also h bound_thd'; reward = dx Gx' + dy Gy':
   |dx| bound_Gx + |dy| bound_Gy + 3 u (|dx Gx'| + |dy Gy'|).
 * residual: dist = || step - stored ||_2, and | ||a|| - ||b|| | <= || a - b ||: || bound_step ||_2 + (d + 4) u dist;
   a workgroup's partial: the sum of its bounds + gamma_(256 + 16) sum dist; a row sum: gamma_(nb + 16) again.
 * normal equations: r = step - stored: e_r = bound_step + u |r|; J_i = (r+ - r-) inv_2e: (e+ + e-) |inv_2e| +
   2 u |J_i|; each of the 13 sums of products a b: sum (e_a |b| + e_b |a| + e_a e_b) + gamma_(d + 256 + nb + 16)
   sum |a b|.

A ratio |got - ref| / bound above 1 is a failure, never a reason for a larger K.
"""
import collections
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = LD(2.0) ** -26                       # the central differences' step
BLOCK, WAVE = 256, 64                      # kStepBlock, kWave

Ref = collections.namedtuple("Ref", "value bound")       # a reference value (np.longdouble) and its bound (float64)


def gamma(j):
    return j * U / (1.0 - j * U)


def ratio(got, ref):
    """max |got - ref.value| / ref.bound over the entries; an entry with bound 0 must be equal.  A NaN or infinite
    `got` gives inf."""
    got = np.asarray(got, dtype=np.float64)
    diff = np.abs(LD(1) * got - ref.value).astype(np.float64)
    bound = np.broadcast_to(np.asarray(ref.bound, dtype=np.float64), diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    q = np.where(np.isfinite(got), q, np.inf)
    return float(np.max(q, initial=0.0))


def solve_ld(A, B):
    """x of A x = B for A [E, K, K], B [E, K]: Gaussian elimination with partial pivoting, in the arrays' type."""
    A, B = A.copy(), B.copy()
    E, K, _ = A.shape
    ar = np.arange(E)
    for j in range(K):
        p = j + np.argmax(np.abs(A[:, j:, j]), axis=1)
        rows, b = A[ar, j].copy(), B[ar, j].copy()
        A[ar, j], B[ar, j] = A[ar, p], B[ar, p]
        A[ar, p], B[ar, p] = rows, b
        f = A[:, j + 1:, j] / A[:, j, j][:, None]
        A[:, j + 1:, j:] -= f[:, :, None] * A[:, j, None, j:]
        B[:, j + 1:] -= f * B[:, j, None]
    X = np.zeros_like(B)
    for i in range(K - 1, -1, -1):
        X[:, i] = (B[:, i] - (A[:, i, i + 1:] * X[:, i + 1:]).sum(axis=1)) / A[:, i, i]
    return X


def _params(E, l, m, k, dtype=LD):
    return tuple(np.broadcast_to(np.asarray(x, dtype=dtype), (E,)) for x in (l, m, k))


def accelerations_ld(n, l, m, k, Gd, s, c, thd, u):
    """The Gym model's (Gdd_x, Gdd_y, thdd_1..n) [E, n + 2].  Gd [E, 2], s, c, thd [E, n], u [E, n - 1]; l, m, k
    scalars or [E].  Computed in the arrays' type (np.longdouble for the reference)."""
    E, K, R = s.shape[0], n + 2, n + 3
    T = s.dtype.type
    l, m, k = _params(E, l, m, k, T)
    AdX, AdY = np.zeros((E, n + 1), T), np.zeros((E, n + 1), T)
    AddX, AddY = np.zeros((E, n + 1, R), T), np.zeros((E, n + 1, R), T)
    GhX, GhY = np.zeros(E, T), np.zeros(E, T)
    GddhX, GddhY = np.zeros((E, R), T), np.zeros((E, R), T)
    for i in range(1, n + 1):                                            # compute_points_speed_acc
        AdX[:, i] = AdX[:, i - 1] - l * thd[:, i - 1] * s[:, i - 1]
        AdY[:, i] = AdY[:, i - 1] + l * thd[:, i - 1] * c[:, i - 1]
        AddX[:, i], AddY[:, i] = AddX[:, i - 1], AddY[:, i - 1]
        AddX[:, i, 2 + i - 1] -= l * s[:, i - 1]
        AddY[:, i, 2 + i - 1] += l * c[:, i - 1]
        AddX[:, i, K] -= l * thd[:, i - 1] ** 2 * c[:, i - 1]
        AddY[:, i, K] -= l * thd[:, i - 1] ** 2 * s[:, i - 1]
        GhX += (AdX[:, i - 1] + AdX[:, i]) / (2 * n)
        GhY += (AdY[:, i - 1] + AdY[:, i]) / (2 * n)
        GddhX += (AddX[:, i - 1] + AddX[:, i]) / (2 * n)
        GddhY += (AddY[:, i - 1] + AddY[:, i]) / (2 * n)
    AdX += (Gd[:, 0] - GhX)[:, None]                                     # change of frame
    AdY += (Gd[:, 1] - GhY)[:, None]
    AddX[:, :, 0] += 1
    AddY[:, :, 1] += 1
    AddX -= GddhX[:, None, :]
    AddY -= GddhY[:, None, :]
    fX, fY = np.zeros((E, n + 1, R), T), np.zeros((E, n + 1, R), T)
    for i in range(1, n + 1):                                            # compute_joint_force
        fX[:, i] = fX[:, i - 1] + m[:, None] * (AddX[:, i - 1] + AddX[:, i]) / 2
        fY[:, i] = fY[:, i - 1] + m[:, None] * (AddY[:, i - 1] + AddY[:, i]) / 2
        nx, ny = -s[:, i - 1], c[:, i - 1]
        gx, gy = (AdX[:, i - 1] + AdX[:, i]) / 2, (AdY[:, i - 1] + AdY[:, i]) / 2
        F = -k * l * (gx * nx + gy * ny)
        fX[:, i, K] -= F * nx
        fY[:, i, K] -= F * ny
    S = np.zeros((E, K, R), T)                                           # compute_dynamic_matrix
    S[:, 0], S[:, 1] = fX[:, n], fY[:, n]
    for i in range(1, n + 1):
        r = S[:, 2 + i - 1]
        r += (l / 2)[:, None] * (c[:, i - 1, None] * (fY[:, i] + fY[:, i - 1])
                                 - s[:, i - 1, None] * (fX[:, i] + fX[:, i - 1]))
        r[:, 2 + i - 1] -= m * l ** 2 / 12
        r[:, K] += k * thd[:, i - 1] * l ** 3 / 12
        if i - 2 >= 0:
            r[:, K] += u[:, i - 2]
        if i - 1 < n - 1:
            r[:, K] -= u[:, i - 1]
    return solve_ld(S[:, :, :K], -S[:, :, K])


def twin_accelerations_ld(n, l, m, k, Gd, s, c, thd, u):
    """The twin model's (Gdd_x, Gdd_y, thdd_1..n) [E, n + 2]: the (5n + 2) system in the unknowns thdd_i | f_0..f_n |
    Gdd_1..n, assembled entry by entry as twin_assemble does and solved densely."""
    E, nn = s.shape[0], 5 * n + 2
    T = s.dtype.type
    l, m, k = _params(E, l, m, k, T)
    nx, ny = -s, c
    g1x, g1y = Gd[:, 0].copy(), Gd[:, 1].copy()                          # compute_friction
    for i in range(1, n + 1):
        sx, sy = np.zeros(E, T), np.zeros(E, T)
        for j in range(i):
            e = T(0.5) if (j == 0 or j == i - 1) else T(1)
            sx += e * thd[:, j] * nx[:, j]
            sy += e * thd[:, j] * ny[:, j]
        g1x -= l / n * sx
        g1y -= l / n * sy
    gx, gy = np.zeros((E, n), T), np.zeros((E, n), T)
    gx[:, 0], gy[:, 0] = g1x, g1y
    for i in range(1, n):
        gx[:, i] = gx[:, i - 1] + l / 2 * thd[:, i - 1] * nx[:, i - 1] + l / 2 * thd[:, i] * nx[:, i]
        gy[:, i] = gy[:, i - 1] + l / 2 * thd[:, i - 1] * ny[:, i - 1] + l / 2 * thd[:, i] * ny[:, i]
    dot = gx * nx + gy * ny
    Fx, Fy = -(k * l)[:, None] * dot * nx, -(k * l)[:, None] * dot * ny
    Mf = -k[:, None] * thd * (l ** 3)[:, None] / 12
    A, B = np.zeros((E, nn, nn), T), np.zeros((E, nn), T)
    for i in range(1, n + 1):                                            # the torque equations
        A[:, i - 1, i - 1] = m * l ** 2 / 12
        A[:, i - 1, n + 2 * i + 0] = l / 2 * s[:, i - 1]
        A[:, i - 1, n + 2 * i + 2] = l / 2 * s[:, i - 1]
        A[:, i - 1, n + 2 * i + 1] = -l / 2 * c[:, i - 1]
        A[:, i - 1, n + 2 * i + 3] = -l / 2 * c[:, i - 1]
        B[:, i - 1] = Mf[:, i - 1]
        if i - 2 >= 0:
            B[:, i - 1] += u[:, i - 2]
        if i - 1 < n - 1:
            B[:, i - 1] -= u[:, i - 1]
    A[:, n, n] = 1
    A[:, n + 1, n + 1] = 1
    for i in range(1, n + 1):                                            # the force balances
        for d, F in enumerate((Fx, Fy)):
            row = n + 2 + 2 * (i - 1) + d
            A[:, row, d + n + 2 * (i - 1)] = 1
            A[:, row, d + n + 2 * i] = -1
            A[:, row, d + 3 * n + 2 * i] = m
            B[:, row] = F[:, i - 1]
    A[:, 3 * n + 2, 3 * n] = 1
    A[:, 3 * n + 3, 3 * n + 1] = 1
    for i in range(1, n):                                                # the joints
        for d in range(2):
            row = 3 * n + 4 + 2 * (i - 1) + d
            A[:, row, d + 3 * n + 2 * i] = 1
            A[:, row, d + 3 * n + 2 * (i + 1)] = -1
            if d == 0:
                A[:, row, i - 1] = -l / 2 * s[:, i - 1]
                A[:, row, i] = -l / 2 * s[:, i]
                B[:, row] = l / 2 * (c[:, i - 1] * thd[:, i - 1] ** 2 + c[:, i] * thd[:, i] ** 2)
            else:
                A[:, row, i - 1] = l / 2 * c[:, i - 1]
                A[:, row, i] = l / 2 * c[:, i]
                B[:, row] = l / 2 * (s[:, i - 1] * thd[:, i - 1] ** 2 + s[:, i] * thd[:, i] ** 2)
    X = solve_ld(A, B)
    out = np.zeros((E, n + 2), T)
    for i in range(1, n + 1):
        out[:, 0] += X[:, 3 * n + 2 * i] / n
        out[:, 1] += X[:, 3 * n + 2 * i + 1] / n
    out[:, 2:] = X[:, :n]
    return out


MODELS = {"gym": accelerations_ld, "twin": twin_accelerations_ld}


def unpack(state, action):
    """state [E, d], action [E, n - 1] as exact doubles -> (n, Gd, s, c, thd, u) in long double."""
    st = LD(1) * np.asarray(state, dtype=np.float64)
    n = (st.shape[1] - 2) // 2
    th = st[:, 2::2]
    return n, st[:, :2], np.sin(th), np.cos(th), st[:, 3::2], LD(1) * np.asarray(action, dtype=np.float64)


def condition(model, n, l, m, k, Gd, s, c, thd, u):
    """(ref [E, n + 2], C [E, n + 2]): C_j = sum_x |d f_j / d x| w_x by central differences (the module's docstring)."""
    f = MODELS[model]
    E = s.shape[0]
    args = dict(Gd=Gd, s=s, c=c, thd=thd, u=u)
    base = f(n, l, m, k, **args)
    tot = np.zeros_like(base)
    for name, a in args.items():
        for j in range(a.shape[1]):
            ap, am = a.copy(), a.copy()
            if name in ("s", "c"):
                ap[:, j] += EPS
                am[:, j] -= EPS
            else:
                ap[:, j] *= 1 + EPS
                am[:, j] *= 1 - EPS
            hi, lo = f(n, l, m, k, **dict(args, **{name: ap})), f(n, l, m, k, **dict(args, **{name: am}))
            tot += np.abs(hi - lo) / (2 * EPS)
    par = dict(zip("lmk", _params(E, l, m, k)))
    for name in "lmk":
        hi, lo = dict(par), dict(par)
        hi[name] = par[name] * (1 + EPS)
        lo[name] = par[name] * (1 - EPS)
        tot += np.abs(f(n, hi["l"], hi["m"], hi["k"], **args) - f(n, lo["l"], lo["m"], lo["k"], **args)) / (2 * EPS)
    return base, tot


def accelerations_ref(model, l, m, k, state, action, K=1.0, cond=None):
    """Ref([E, n + 2], bound [E, 1]) of the accelerations, and sharpness [E] = max_j C_j / max_j |ref_j|.  cond: what
    condition() gave for these arguments (it does not depend on K)."""
    if cond is None:
        n, Gd, s, c, thd, u = unpack(state, action)
        cond = condition(model, n, l, m, k, Gd, s, c, thd, u)
    ref, C = cond
    top = np.abs(ref).max(axis=1)
    bound = (K * U * (C + np.abs(ref)).max(axis=1)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sharp = (C.max(axis=1) / top).astype(np.float64)
    return Ref(ref, bound[:, None]), sharp


def euler(model, h, direction, state, acc, xp=LD):
    """(next [E, d], reward [E]) from the accelerations [E, n + 2]: explicit Euler for the Gym model (the angle moves
    with the OLD thetadot), semi-implicit for the twin (with the new one).  xp: the type it is computed in."""
    st = np.asarray(state, dtype=np.float64).astype(xp)
    acc, h = np.asarray(acc).astype(xp), xp(h)
    out = np.empty_like(st)
    out[:, :2] = st[:, :2] + h * acc[:, :2]
    out[:, 3::2] = st[:, 3::2] + h * acc[:, 2:]
    out[:, 2::2] = st[:, 2::2] + h * (out[:, 3::2] if model == "twin" else st[:, 3::2])
    return out, out[:, 0] * xp(direction[0]) + out[:, 1] * xp(direction[1])


def step_ld(model, l, m, k, h, direction, state, action):
    """(next [E, d], reward [E]) in long double, no bounds."""
    n, Gd, s, c, thd, u = unpack(state, action)
    return euler(model, h, direction, state, MODELS[model](n, l, m, k, Gd, s, c, thd, u))


def step_ref(model, l, m, k, h, direction, state, action, K=1.0, cond=None):
    """{"accel": Ref [E, n + 2], "next": Ref [E, d], "reward": Ref [E], "sharp": [E]} of one step."""
    acc, sharp = accelerations_ref(model, l, m, k, state, action, K, cond)
    nxt, rew = euler(model, h, direction, state, acc.value)
    st = np.abs(np.asarray(state, dtype=np.float64))
    ha = np.abs(float(h) * acc.value).astype(np.float64)
    hb = abs(float(h)) * acc.bound                                        # [E, 1]
    bound = np.empty(st.shape)
    bound[:, :2] = hb + 2 * U * (st[:, :2] + ha[:, :2])
    bound[:, 3::2] = hb + 2 * U * (st[:, 3::2] + ha[:, 2:])
    if model == "twin":
        moved = np.abs(float(h) * nxt[:, 3::2]).astype(np.float64)
        bound[:, 2::2] = abs(float(h)) * bound[:, 3::2] + 2 * U * (st[:, 2::2] + moved)
    else:
        bound[:, 2::2] = 2 * U * (st[:, 2::2] + abs(float(h)) * st[:, 3::2])
    dx, dy = abs(float(direction[0])), abs(float(direction[1]))
    g = np.abs(nxt[:, :2]).astype(np.float64)
    rb = dx * bound[:, 0] + dy * bound[:, 1] + 3 * U * (dx * g[:, 0] + dy * g[:, 1])
    return {"accel": acc, "next": Ref(nxt, bound), "reward": Ref(rew, rb), "sharp": sharp}


# ------------------------------------------------------------------------------------------------------------
# the residual kernels

def blocks(T):
    return (T + BLOCK - 1) // BLOCK


def distances(nxt, stored, with_gdot=True):
    """Ref [T]: || next - stored ||_2 per transition from a step's Ref [T, d].  with_gdot = False is the wrong
    restatement that leaves the two Gdot components out."""
    d = nxt.value.shape[1]
    diff = nxt.value - LD(1) * np.asarray(stored, dtype=np.float64)
    if not with_gdot:
        diff = diff[:, 2:]
    dist = np.sqrt((diff * diff).sum(axis=1))
    bound = np.sqrt((nxt.bound ** 2).sum(axis=1)) + (d + 4) * U * dist.astype(np.float64)
    return Ref(dist, bound)


def partials(dist):
    """Ref [blocks(T)]: the per-workgroup sums of a distances Ref."""
    T, nb = dist.value.shape[0], blocks(dist.value.shape[0])
    pad = nb * BLOCK - T
    v = np.concatenate([dist.value, np.zeros(pad, LD)]).reshape(nb, BLOCK).sum(axis=1)
    b = np.concatenate([dist.bound, np.zeros(pad)]).reshape(nb, BLOCK).sum(axis=1)
    return Ref(v, b + gamma(BLOCK + 16) * v.astype(np.float64))


def row_total(part):
    """Ref (scalar): the sum of a partials Ref."""
    v = part.value.sum()
    return Ref(v, float(part.bound.sum() + gamma(len(part.value) + 16) * float(np.abs(part.value).sum())))


def row_sum_fixed_order(row):
    """The documented order of residual_rows_sum_kernel in float64: lane l adds row[l], row[l + 64], ... in turn from
    0.0, then the lane sums pair up as __shfl_down(., 32), (., 16), ..., (., 1) do.  Exact restatement: bit for bit."""
    row = np.asarray(row, dtype=np.float64)
    lanes = np.zeros(WAVE)
    for b0 in range(0, len(row), WAVE):
        chunk = row[b0:b0 + WAVE]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    t = lanes.copy()
    off = WAVE // 2
    while off:
        shifted = np.concatenate([t[off:], t[WAVE - off:]])   # __shfl_down beyond the wave returns the lane's own
        t = t + shifted
        off //= 2
    return t[0]


def normal_ref(steps, stored, inv_2e):
    """Ref [13] (or [1] with one point) of r.r | J^T J | J^T r over the transitions: steps = the 7 (or 1) "next" Refs
    [T, d] at the points centre, +e0, -e0, +e1, -e1, +e2, -e2 (Gym model); inv_2e [3]."""
    stored = LD(1) * np.asarray(stored, dtype=np.float64)
    T, d = stored.shape

    def res(s):
        r = s.value - stored
        return r, s.bound + U * np.abs(r).astype(np.float64)
    r0, e0 = res(steps[0])
    cols = [(r0, e0)]
    for i in range((len(steps) - 1) // 2):
        (rp, ep), (rm, em) = res(steps[1 + 2 * i]), res(steps[2 + 2 * i])
        J = (rp - rm) * LD(inv_2e[i])
        e = (ep + em) * abs(float(inv_2e[i]))
        # the Gym model's new angle th + h thd depends on no parameter: every point computes the same number from the
        # same inputs, the two residuals are equal and this entry of J is exactly 0, here and in any kernel
        e[:, 2::2] = 0.0
        cols.append((J, e + 2 * U * np.abs(J).astype(np.float64)))
    g = gamma(d + BLOCK + blocks(T) + 16)

    def dot(a, b):
        (x, ex), (y, ey) = cols[a], cols[b]
        ax, ay = np.abs(x).astype(np.float64), np.abs(y).astype(np.float64)
        return (x * y).sum(), float((ex * ay + ey * ax + ex * ey).sum() + g * (ax * ay).sum())
    if len(cols) == 1:
        pairs = [(0, 0)]
    else:
        pairs = [(0, 0)] + [(a, b) for a in (1, 2, 3) for b in (1, 2, 3)] + [(a, 0) for a in (1, 2, 3)]
    vals = [dot(a, b) for a, b in pairs]
    return Ref(np.array([v for v, _ in vals], dtype=LD), np.array([b for _, b in vals]))


def k_from(r_oracle):
    """K = 4 R_oracle rounded up to a power of two."""
    return float(2.0 ** math.ceil(math.log2(4.0 * r_oracle)))
