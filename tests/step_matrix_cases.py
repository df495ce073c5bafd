"""Generated cases for the step family (csrc/swimmer_step.hip): sw_step_f64, sw_accel_f64, sw_reset_f64, the four
sw_step_residual* entry points and sw_env1_*, and the list of the 115 kernels they dispatch to.  Inputs and references
only: nothing here touches the GPU.  The references and bounds are tests/step_reference.py's;
tests/test_step_matrix_cpu.py shows on the fp64 oracle alone that the cases can catch what they are for and fixes K,
tests/test_step_matrix_gpu.py holds the kernels to them.

STATES.  Per (model, n, parameter set) one batch of 513 environments in a fixed interleaved order, so that every prefix
(the batch sizes 1, 63, 64, 65, 255, 256, 257, 513: a partial wave, a full wave, a partial workgroup, two workgroups
and one lane) mixes the regimes:
  calm      angles in (-pi, pi), |thetadot| <= 2, |u| <= 5, |Gdot| <= 0.5, and well conditioned (CALM_LIMIT)
  fast      |thetadot| <= 300
  torque    |u| <= 1e4
  straight  every angle within 1e-3 of a common one
  folded    angles alternating by pi, within 1e-3
  edges     every angle from EDGE_ANGLES: k pi/4 and k pi/2 rounded to double and their neighbours at +-1 and +-2 ulp, k
            in {0, +-1 .. +-4, +-(2^20 + 1), +-(2^30 + 3), the largest k below the range limit}, +-0, 5e-324, 1e-300
            and +-nextafter(3e9, 0); consecutive environments walk through the list
The Gym model has 513 different states; the twin's reference solves a (5n + 2) system per perturbed input, so its batch
repeats 171 different states three times (neighbouring environments still differ: a wrong index shows).

STATUS CASES (include/swimmer_hip.h): lanes 0, 63, 64 and n_env - 1 of a 257-environment calm batch carry the fault.
  |theta| == 3.0e9 exactly, -3.0e9, 5e9, +-inf: RANGE (|theta| >= 3e9), the whole column NaN, hence NONFINITE too
  NaN angle: NONFINITE and not RANGE (NaN >= 3e9 is false)
  NaN / inf in a thetadot, in Gdot, in an action: NONFINITE, not RANGE
The SINGULAR bit of a column that is not finite is left open (a pivot of NaN is "not finite"; one formed from an angle
out of range is undefined).  Every other lane: status 0 exactly, and inside its bounds.
"""
import collections
import functools
import math

import numpy as np

import step_reference as sr
from step_reference import LD, Ref, U      # noqa: F401 (re-exported for the tests)

NS = tuple(range(2, 9))
MODELS = ("gym", "twin")
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
N_ENV = SIZES[-1]
RESET_SIZES = (1, 255, 257)
DIRECTION = (0.6, -0.8)
GYM_SETS = (("default", (1.0, 1.0, 10.0, 1e-3)), ("realworld", (0.8, 1.2, 10.2, 1e-3)),
            ("odd", (1.3, 0.7, 4.5, 2.5e-3)))                 # conftest.PARAM_SETS, with DIRECTION
TWIN_SETS = ((1.0, 1.0, 10.0, 0.01, (1.0, 0.0)), (0.8, 1.2, 10.2, 0.003, (0.6, -0.8)))   # tests/test_twin.py
REGIMES = ("calm", "fast", "torque", "straight", "folded", "edges")
UNIQUE = {"gym": (83, 98), "twin": (24, 51)}                  # states per regime, and in the edge regime
CALM_LIMIT = 1e-13 / 32                                       # of h u max_j (C_j + |ref_j|) in the calm regime
ANGLE_LIMIT = 3.0e9                                           # kAngleLimit
STATUS_SINGULAR, STATUS_NONFINITE, STATUS_RANGE = 1, 2, 4
STATUS_N_ENV, STATUS_LANES = 257, (0, 63, 64, 256)
POISON = -7.25e77                                             # guards and never-written entries
GUARD = 64
RES_SIZES = (1, 255, 256, 257, 1000)
RES_T = 1024                                                  # the NT pattern; the sizes above are its prefixes
STORES = ("noise", "rounded", "moved")
SET_LENGTHS = (1, 255, 256, 257, 700)
SET_OF_CANDIDATE = (0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 4, 4, 4)  # set 3 has no candidate; the first group of 8
                                                               # straddles sets 0 and 1, the second 1, 2 and 4
ACTIVE = (1, 1, 0, 1, 1)
N_POINTS = (1, 7)
POP_CANDIDATES = 9                                            # a full group of 8 and a partial one
NT_PATTERN, NT_TAIL = 1024, 513
STREAM_BYTES = 256 << 20                                      # kStepStreamBytes
# K of the acceleration bound, per model: 4 R_oracle rounded up to a power of two, R_oracle the fp64 oracle's worst
# ratio under K = 1 over every case below.  tests/test_step_matrix_cpu.py measures R_oracle and fails when this is
# not what it gives; a GPU ratio above 1 is never answered here.
K_MEASURED = {"gym": 32.0, "twin": 16.0}

Inst = collections.namedtuple("Inst", "symbol entry n twin nt n_point accel")


def _sym(name, *args):
    """The Itanium spelling of a kernel's (anonymous-namespace) name with its template arguments, up to the E that
    closes the nested name: no other kernel's symbol contains it."""
    spell = "".join(f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in args)
    return f"_GLOBAL__N_1{len(name)}{name}" + (f"I{spell}EE" if args else "E")


KERNEL_NAMES = ("step_kernel", "accel_kernel", "step_residual_kernel", "step_residual_pop_kernel",
                "step_residual_sets_kernel", "step_residual_normal_sets_kernel", "env1_kernel", "reset_kernel",
                "residual_rows_sum_kernel", "residual_set_rows_sum_kernel")
COUNTS = (21, 14, 14, 14, 7, 14, 28, 1, 1, 1)


def _instantiations():
    out = []
    for n in NS:
        # NT "forced": only SWIMMER_STEP_NT=1 (read once per process) reaches it at test sizes; the twin has no NT form
        out += [Inst(_sym("step_kernel", n, False, False), "sw_step_f64", n, False, None, None, None),
                Inst(_sym("step_kernel", n, False, True), "sw_step_f64", n, False, "forced", None, None),
                Inst(_sym("step_kernel", n, True, False), "sw_step_f64", n, True, None, None, None)]
        out += [Inst(_sym("accel_kernel", n, t), "sw_accel_f64", n, t, None, None, None) for t in (False, True)]
        # NT "size": more than 256 MiB of traffic in the launch
        for name, entry in (("step_residual_kernel", "sw_step_residual_f64"),
                            ("step_residual_pop_kernel", "sw_step_residual_pop_f64")):
            out += [Inst(_sym(name, n, nt), entry, n, False, "size" if nt else None, None, None)
                    for nt in (False, True)]
        out.append(Inst(_sym("step_residual_sets_kernel", n), "sw_step_residual_sets_f64", n, False, None, None, None))
        out += [Inst(_sym("step_residual_normal_sets_kernel", n, np_), "sw_step_residual_normal_sets_f64", n, False,
                     None, np_, None) for np_ in N_POINTS]
        out += [Inst(_sym("env1_kernel", n, t, a), "sw_env1_accel" if a else "sw_env1_step", n, t, None, None, a)
                for t in (False, True) for a in (False, True)]
    out += [Inst(_sym("reset_kernel"), "sw_reset_f64", None, None, None, None, None),
            Inst(_sym("residual_rows_sum_kernel"), "sw_step_residual_pop_f64", None, None, None, None, None),
            Inst(_sym("residual_set_rows_sum_kernel"), "sw_step_residual_sets_f64", None, None, None, None, None)]
    return tuple(out)


INSTANTIATIONS = _instantiations()


def find(name, **kw):
    """The entries of INSTANTIATIONS of kernel `name` whose fields equal kw."""
    head = f"_GLOBAL__N_1{len(name)}{name}"
    return [i for i in INSTANTIATIONS if i.symbol.startswith(head) and i.symbol[len(head)] in "IE"
            and all(getattr(i, k) == v for k, v in kw.items())]


def reached_by():
    """{GPU test name: the instantiations its parametrisation launches}: tests/test_step_matrix_gpu.py parametrises
    over the same NS, MODELS and N_POINTS, and asserts that these names are its tests."""
    rows = find("residual_rows_sum_kernel")
    set_rows = find("residual_set_rows_sum_kernel")
    return {
        "test_step_accel_within_bounds": [i for n in NS for t in (False, True)
                                          for i in find("step_kernel", n=n, twin=t, nt=None)
                                          + find("accel_kernel", n=n, twin=t)],
        "test_reset": find("reset_kernel"),
        "test_nt_step_forms_in_a_child_process": [i for n in NS for i in find("step_kernel", n=n, nt="forced")],
        "test_env1_is_the_batched_kernel": [i for n in NS for t in (False, True)
                                            for i in find("env1_kernel", n=n, twin=t)],
        "test_residual_single": [i for n in NS for i in find("step_residual_kernel", n=n, nt=None)],
        "test_residual_nt_forms": [i for n in NS for i in find("step_residual_kernel", n=n, nt="size")
                                   + find("step_residual_pop_kernel", n=n, nt="size")] + rows,
        "test_residual_population": [i for n in NS for i in find("step_residual_pop_kernel", n=n, nt=None)] + rows,
        "test_residual_sets": [i for n in NS for i in find("step_residual_sets_kernel", n=n)] + set_rows,
        "test_residual_normal_sets": [i for n in NS for np_ in N_POINTS
                                      for i in find("step_residual_normal_sets_kernel", n=n, n_point=np_)] + set_rows,
    }


def _seed(*parts):
    s = 0
    for x in parts:
        s = (s * 1000003 + int(x) + 7) % (2 ** 32)
    return s


# ------------------------------------------------------------------------------------------------------------
# the angle edge set

PI_LD = LD(4) * np.arctan(LD(1))


def _edge_angles():
    out = []
    for div in (4, 2):
        unit = PI_LD / div
        k_max = int(math.floor(ANGLE_LIMIT / float(unit)))
        while float(LD(k_max) * unit) >= ANGLE_LIMIT:
            k_max -= 1
        ks = [0] + [s * k for k in (1, 2, 3, 4, 2 ** 20 + 1, 2 ** 30 + 3, k_max) for s in (1, -1)]
        for k in ks:
            x = np.float64(LD(k) * unit)
            lo, hi = x, x
            out.append(x)
            for _ in range(2):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
                out += [lo, hi]
    edge = np.nextafter(ANGLE_LIMIT, 0.0)
    out += [0.0, -0.0, 5e-324, 1e-300, edge, -edge]
    out = np.array(out, dtype=np.float64)
    return out[np.abs(out) < ANGLE_LIMIT]


EDGE_ANGLES = _edge_angles()


# ------------------------------------------------------------------------------------------------------------
# states

def param_sets(model):
    """[(l, m, k, h, direction)] of a model."""
    return [p + (DIRECTION,) for _, p in GYM_SETS] if model == "gym" else list(TWIN_SETS)


def _unique_states(model, n, pi):
    per, edges = UNIQUE[model]
    rs = np.random.RandomState(_seed(MODELS.index(model), n, pi, 1))
    count = 5 * per + edges
    d = 2 * n + 2
    st = np.empty((count, d))
    st[:, :2] = rs.uniform(-0.5, 0.5, (count, 2))
    st[:, 2::2] = rs.uniform(-np.pi, np.pi, (count, n))
    st[:, 3::2] = rs.uniform(-2, 2, (count, n))
    ac = rs.uniform(-5, 5, (count, n - 1))
    regime = np.repeat(np.arange(6), [per] * 5 + [edges])
    st[regime == 1, 3::2] = rs.uniform(-300, 300, (per, n))
    ac[regime == 2] = rs.uniform(-1e4, 1e4, (per, n - 1))
    st[regime == 3, 2::2] = rs.uniform(-np.pi, np.pi, (per, 1)) + rs.uniform(-1e-3, 1e-3, (per, n))
    st[regime == 4, 2::2] = (rs.uniform(-np.pi, np.pi, (per, 1)) + np.pi * (np.arange(n) % 2)
                             + rs.uniform(-1e-3, 1e-3, (per, n)))
    walk = (pi * edges * n + np.arange(edges * n)) % len(EDGE_ANGLES)
    st[regime == 5, 2::2] = EDGE_ANGLES[walk].reshape(edges, n)
    # calm also means well conditioned (the twin's system at n = 4 is not, for some chains): a calm draw whose
    # acceleration bound at K = 1, times h, is above CALM_LIMIT is drawn again
    l, m, k, h, _ = param_sets(model)[pi]
    calm = np.flatnonzero(regime == 0)
    for _ in range(50):
        ref, C = sr.condition(model, n, l, m, k, *sr.unpack(st[calm], ac[calm])[1:])
        bad = calm[h * U * (C + np.abs(ref)).max(axis=1).astype(np.float64) > CALM_LIMIT]
        if not len(bad):
            break
        st[bad, 2::2] = rs.uniform(-np.pi, np.pi, (len(bad), n))
        st[bad, 3::2] = rs.uniform(-2, 2, (len(bad), n))
        ac[bad] = rs.uniform(-5, 5, (len(bad), n - 1))
        calm = bad
    else:
        raise AssertionError("no well-conditioned calm states")
    return st, ac, regime


@functools.lru_cache(maxsize=None)
def case(model, n, pi):
    """dict(model, n, l, m, k, h, direction, state [513, d], action [513, n - 1], regime [513]: index into REGIMES,
    unique: (state, action) of the different states, index [513]: which of them an environment holds)."""
    l, m, k, h, direction = param_sets(model)[pi]
    st, ac, regime = _unique_states(model, n, pi)
    index = (np.arange(N_ENV) * 97) % len(st)        # 97 is coprime to 513 and to 171: a walk through all of them
    return dict(model=model, n=n, l=l, m=m, k=k, h=h, direction=direction, state=st[index], action=ac[index],
                regime=regime[index], unique=(st, ac), index=index)


@functools.lru_cache(maxsize=None)
def _condition(model, n, pi):
    c = case(model, n, pi)
    return sr.condition(model, n, c["l"], c["m"], c["k"], *sr.unpack(*c["unique"])[1:])


@functools.lru_cache(maxsize=None)
def reference(model, n, pi, K=None):
    """The step's Refs of case(model, n, pi), [513, ...] each: accel, next, reward, and sharp [513].  K: the bound's
    factor, the model's measured one when None."""
    c = case(model, n, pi)
    ref = sr.step_ref(model, c["l"], c["m"], c["k"], c["h"], c["direction"], *c["unique"],
                      K=K_MEASURED[model] if K is None else K, cond=_condition(model, n, pi))
    ix = c["index"]
    return {"sharp": ref["sharp"][ix],
            **{key: Ref(ref[key].value[ix], ref[key].bound[ix]) for key in ("accel", "next", "reward")}}


def oracle_outputs(model, n, pi, scale_k=1.0, scale_l=1.0, direction=None, state=None, action=None):
    """(accel [E, n + 2], next [E, d], reward [E]) of the fp64 oracle on case(model, n, pi) (or on state / action)."""
    import oracle
    c = case(model, n, pi)
    st = c["state"] if state is None else state
    ac = c["action"] if action is None else action
    op = oracle.OracleParams.make(n, c["l"] * scale_l, c["m"], c["k"] * scale_k, c["h"], direction or c["direction"])
    acc_f = oracle.accelerations if model == "gym" else oracle.twin_accelerations
    step_f = oracle.step_batch if model == "gym" else oracle.twin_step_batch
    acc = np.array([np.concatenate(acc_f(op, st[e], ac[e])) for e in range(len(st))])
    nxt, rew = step_f(op, st, ac)
    return acc, nxt, rew


def reset_state(model, n, n_env):
    """The oracle's reset state [n_env, d] (twin: env_start's all 0.001)."""
    import oracle
    if model == "twin":
        return np.full((n_env, 2 * n + 2), 0.001)
    return np.tile(oracle.reset(oracle.OracleParams.make(n)), (n_env, 1))


# ------------------------------------------------------------------------------------------------------------
# status cases

STATUS_KINDS = (                            # (name, field, value, bits that must be set, bits that must be clear)
    ("angle_at_limit", "angle", ANGLE_LIMIT, 6, 0), ("angle_at_minus_limit", "angle", -ANGLE_LIMIT, 6, 0),
    ("angle_5e9", "angle", 5e9, 6, 0), ("angle_inf", "angle", np.inf, 6, 0),
    ("angle_minus_inf", "angle", -np.inf, 6, 0),
    ("angle_nan", "angle", np.nan, 2, 4),
    ("thetadot_nan", "thetadot", np.nan, 2, 4), ("thetadot_inf", "thetadot", np.inf, 2, 4),
    ("gdot_nan", "gdot", np.nan, 2, 4), ("gdot_inf", "gdot", -np.inf, 2, 4),
    ("action_nan", "action", np.nan, 2, 4), ("action_inf", "action", np.inf, 2, 4))


def status_case(model, n, kind):
    """(state [257, d], action [257, n - 1], lanes) with the fault of STATUS_KINDS[kind] in lanes 0, 63, 64, 256 of the
    first 257 environments of case(model, n, 0); every other lane keeps its state, and so reference(model, n, 0)'s
    Refs."""
    c = case(model, n, 0)
    st, ac = c["state"][:STATUS_N_ENV].copy(), c["action"][:STATUS_N_ENV].copy()
    _, field, value, _, _ = STATUS_KINDS[kind]
    for j, e in enumerate(STATUS_LANES):
        i = (j + kind) % n
        if field == "angle":
            st[e, 2 + 2 * i] = value
        elif field == "thetadot":
            st[e, 3 + 2 * i] = value
        elif field == "gdot":
            st[e, j % 2] = value
        else:
            ac[e, i % (n - 1)] = value
    return st, ac, STATUS_LANES


# ------------------------------------------------------------------------------------------------------------
# the residual kernels (Gym model)

def tile(a, T):
    """T rows: row t is row t mod len(a)."""
    return a[np.arange(T) % len(a)]


@functools.lru_cache(maxsize=None)
def transitions(n, pi, T=RES_T):
    """dict(state [T, d], action [T, n - 1], stores {name: [T, d]}) on the states of case("gym", n, pi), repeated
    beyond 513 (every repeat has noise of its own):
      noise    the reference's next state + N(0, 1e-3)
      rounded  the reference's next state rounded to double: the distance is at rounding level, the bound decides
      moved    `rounded` with one transition per workgroup moved by 1e6 in one component: absorption in the sum"""
    c = case("gym", n, pi)
    nxt = tile(reference("gym", n, pi)["next"].value.astype(np.float64), T)
    rs = np.random.RandomState(_seed(n, pi, T, 2))
    moved = nxt.copy()
    for b in range(sr.blocks(T)):
        t = b * sr.BLOCK + (17 * (b + 1)) % sr.BLOCK
        if t < T:
            moved[t, b % nxt.shape[1]] += 1e6
    return dict(state=tile(c["state"], T), action=tile(c["action"], T),
                stores={"noise": nxt + rs.normal(0.0, 1e-3, nxt.shape), "rounded": nxt, "moved": moved})


def step_refs_of(n, pi, T, K=None, l=None, m=None, k=None):
    """The "next" Ref [T, d] of transitions(n, pi)'s first T states, at the set's parameters or at (l, m, k)."""
    c = case("gym", n, pi)
    if l is None:
        ref = reference("gym", n, pi, K)["next"]
    else:
        ref = sr.step_ref("gym", l, m, k, c["h"], c["direction"], c["state"][:min(T, N_ENV)],
                          c["action"][:min(T, N_ENV)], K=K_MEASURED["gym"] if K is None else K)["next"]
    ix = np.arange(T) % N_ENV
    return Ref(ref.value[ix], ref.bound[ix])


def residual_reference(n, pi, store, T, K=None, with_gdot=True):
    """Ref [blocks(T)] of sw_step_residual_f64's partials on the first T transitions against `store`."""
    nxt = step_refs_of(n, pi, T, K)
    return sr.partials(sr.distances(nxt, transitions(n, pi)["stores"][store][:T], with_gdot))


@functools.lru_cache(maxsize=None)
def set_transitions(n, pi):
    """dict(state, action, stored) of the sets' concatenated transitions (sum(SET_LENGTHS) of them, the `noise`
    store), again the states of case("gym", n, pi) repeated."""
    T = int(sum(SET_LENGTHS))
    c = case("gym", n, pi)
    rs = np.random.RandomState(_seed(n, pi, T, 3))
    nxt = tile(reference("gym", n, pi)["next"].value.astype(np.float64), T)
    return dict(state=tile(c["state"], T), action=tile(c["action"], T), stored=nxt + rs.normal(0.0, 1e-3, nxt.shape))


def normal_reference(n, pi, s, n_point, K=None):
    """Ref [13] or [1] of set s of set_transitions(n, pi) at normal_points(n, pi, n_point).  The six points around
    the centre differ from it by 1e-6 in one constant: their condition term is the centre's (which costs 8n + 9
    evaluations of the model per point) times 1 + 1e-3, their values are evaluated at the points themselves."""
    c, tr = case("gym", n, pi), set_transitions(n, pi)
    b0 = int(set_begin()[s])
    sl = slice(b0, b0 + SET_LENGTHS[s])
    st, ac = tr["state"][sl], tr["action"][sl]
    points, inv = normal_points(n, pi, n_point)
    K = K_MEASURED["gym"] if K is None else K
    args = sr.unpack(st, ac)[1:]
    _, C = sr.condition("gym", n, *points[s][0], *args)
    steps = []
    for j, (l, m, k) in enumerate(points[s]):
        cond = (sr.accelerations_ld(n, l, m, k, *args), C * (1 if j == 0 else 1 + 1e-3))
        steps.append(sr.step_ref("gym", l, m, k, c["h"], c["direction"], st, ac, K=K, cond=cond)["next"])
    return sr.normal_ref(steps, tr["stored"][sl], inv[s])


@functools.lru_cache(maxsize=None)
def oracle_ratios(model, n, pi):
    """The fp64 oracle on case(model, n, pi): (its acceleration ratio under K = 1 per environment [513], its
    next-state ratio and its reward ratio under the measured K)."""
    ref, one = reference(model, n, pi), reference(model, n, pi, 1.0)
    acc, nxt, rew = oracle_outputs(model, n, pi)
    diff = np.abs(LD(1) * acc - one["accel"].value).astype(np.float64)
    return (diff / one["accel"].bound).max(axis=1), sr.ratio(nxt, ref["next"]), sr.ratio(rew, ref["reward"])


def r_oracle(model):
    """The oracle's worst acceleration ratio under K = 1 over every case of the model."""
    return float(max(oracle_ratios(model, n, pi)[0].max() for n in NS for pi in range(len(param_sets(model)))))


def candidates(n, pi, count):
    """[count, 3] = (l_i, m_i, k): the set's parameters moved by up to a few per cent, every candidate differently."""
    c = case("gym", n, pi)
    j = np.arange(count)[:, None]
    return np.array([c["l"], c["m"], c["k"]]) * (1.0 + 0.01 * j * np.array([1.0, -0.7, 1.3]))


def set_begin():
    return np.concatenate([[0], np.cumsum(SET_LENGTHS)]).astype(np.int64)


def to_constants(m_i, l_i, k):
    """(k l / m, m l^2, k / m): ars/cmaes.py's coordinates of the refinement."""
    return np.array([k * l_i / m_i, m_i * l_i * l_i, k / m_i])


def from_constants(u):
    l_i = u[0] / u[2]
    m_i = u[1] / (l_i * l_i)
    return np.array([m_i, l_i, u[2] * m_i])


def normal_points(n, pi, n_point):
    """(points [n_set, n_point, 3] = (l_i, m_i, k), inv_2e [n_set, 3]) as Estimator._residual_normal builds them:
    centre u = to_constants(m, l, k), then u +- e_i with e_i = 1e-6 |u_i|, inv_2e_i = 1 / (2 e_i).  Set s is centred
    on the case's parameters moved by s per cent."""
    c = case("gym", n, pi)
    points, inv = [], []
    for s in range(len(SET_LENGTHS)):
        u = to_constants(c["m"] * (1 + 0.01 * s), c["l"] * (1 - 0.01 * s), c["k"] * (1 + 0.02 * s))
        us = [u]
        e = 1e-6 * np.abs(u)
        for i in range(3):
            step = np.zeros(3)
            step[i] = e[i]
            us += [u + step, u - step]
        points.append([from_constants(v)[[1, 0, 2]] for v in us[:n_point]])
        inv.append(1.0 / (2 * e))
    return np.array(points), np.array(inv)


def nt_transitions(n):
    """The number of transitions q * 1024 + 513 with the smallest q whose launch streams more than 256 MiB."""
    per = 8 * (2 * (2 * n + 2) + n)
    need = STREAM_BYTES // per + 1                   # the smallest n_env with n_env * per > STREAM_BYTES
    return -(-(need - NT_TAIL) // NT_PATTERN) * NT_PATTERN + NT_TAIL
