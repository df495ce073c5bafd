"""The return codes of the rollout entry points' argument checks, row by row, and which check comes first where two
arguments are wrong at once.  Every row fails (or returns early) before the entry point touches the device, so the
test needs no GPU and dummy non-null pointers will do; no row may expect SW_ERR_LAUNCH.  The expected codes are what
the library returned before the launch layer was given its launcher tables: they pin the order of the checks."""
import ctypes

import pytest

P = ctypes.c_void_p(8)          # a non-null pointer nobody dereferences
NAN = float("nan")
OK, NULL, SEGMENTS, SIZE, PARAM, LAUNCH = range(6)
MAX_AGENTS, MAX_DIRS = 65535, 1 << 23

# entry point -> its arguments in order, with values that would pass every check
SIGNATURES = {
    "sw_rollout_f64": [("p", "n3"), ("n_roll", 18), ("H", 5), ("policies", P), ("mean", None), ("inv_std", None),
                       ("state0", None), ("returns", P), ("traj", None), ("final_state", None), ("moments", None),
                       ("status", None), ("stream", None)],
    "sw_ars_rollouts_f64": [("p", "n3"), ("dir_begin", 0), ("n_dir", 9), ("H", 5), ("policy", P), ("deltas", P),
                            ("nu", 0.01), ("mean", None), ("inv_std", None), ("returns", P), ("traj", None),
                            ("moments", None), ("status", None), ("stream", None)],
    "sw_ars_gate_f64": [("p", "n3"), ("dir_begin", 0), ("n_dir", 9), ("H", 5), ("policy", P), ("deltas", P),
                        ("nu", 0.01), ("mean", None), ("inv_std", None), ("sim_thresh", 0.0), ("admit", P),
                        ("returns", P), ("status", None), ("stream", None)],
    "sw_safe_rollouts_f64": [("p", "n3"), ("sim", "n3"), ("n_roll", 18), ("H", 5), ("policies", P), ("cost_kind", 0),
                             ("cost_index", 3), ("sim_thresh", 0.3), ("real_thresh", 0.3), ("returns", P),
                             ("traj", None), ("first_refused", None), ("violations", None), ("status", None),
                             ("stream", None)],
    "sw_ars_rollouts_multi_f64": [("p", "n3"), ("n_agent", 2), ("n_dir", 9), ("H", 5), ("policy", P), ("deltas", P),
                                  ("nu", 0.01), ("mean", None), ("inv_std", None), ("returns", P), ("moments", None),
                                  ("status", None), ("stream", None)],
    "sw_ars_gate_multi_f64": [("p", "n3"), ("n_agent", 2), ("n_dir", 9), ("H", 5), ("policy", P), ("deltas", P),
                              ("nu", 0.01), ("mean", None), ("inv_std", None), ("sim", P), ("sim_thresh", P),
                              ("admit", P), ("returns", P), ("status", None), ("stream", None)],
    "sw_ars_rollouts_multi_counted_f64": [("p", "n3"), ("n_agent", 2), ("n_dir", 9), ("count", P), ("H", 5),
                                          ("policy", P), ("deltas", P), ("nu", 0.01), ("mean", None),
                                          ("inv_std", None), ("returns", P), ("moments", None), ("status", None),
                                          ("stream", None)],
    "sw_safe_ars_rollouts_multi_f64": [("p", "n3"), ("n_agent", 2), ("n_dir", 9), ("H", 5), ("policy", P),
                                       ("deltas", P), ("nu", 0.01), ("gated", P), ("sim", P), ("sim_thresh", P),
                                       ("real_thresh", P), ("cost_kind", 0), ("cost_index", 3), ("returns", P),
                                       ("cost_trace", None), ("cost_max", None), ("first_refused", None),
                                       ("violations", None), ("status", None), ("stream", None)],
}

# parameter sets by name ("null": no sw_params at all)
PARAMS = {
    "n3": dict(n=3), "n4": dict(n=4), "n9": dict(n=9), "n1": dict(n=1), "bad_l": dict(n=3, l_i=0.0),
    "neg_l": dict(n=3, l_i=-1.0), "nan_k": dict(n=3, k=NAN), "bad_flags": dict(n=3, flags=64),
    "split_and_v1": dict(n=3, flags=8 | 16), "lane": dict(n=3, flags=1), "twin": dict(n=3, flags=4),
}

BAD_PARAMS = [(dict(p="null"), NULL), (dict(p="n9"), SEGMENTS), (dict(p="n1"), SEGMENTS), (dict(p="bad_l"), PARAM),
              (dict(p="neg_l"), PARAM), (dict(p="nan_k"), PARAM), (dict(p="bad_flags"), PARAM),
              (dict(p="split_and_v1"), PARAM)]
MEAN_XOR = [(dict(mean=P), NULL), (dict(inv_std=P), NULL)]
# a launch of 2^32 threads or more: only the lane form gets there (64 slots per 64-thread workgroup)
TOO_MANY_THREADS = [dict(n_agent=MAX_AGENTS, n_dir=MAX_DIRS), dict(n_agent=MAX_AGENTS, n_dir=32800),
                    dict(n_agent=MAX_AGENTS, n_dir=MAX_DIRS, p="lane"), dict(n_agent=MAX_AGENTS, n_dir=MAX_DIRS, p="n4"),
                    dict(n_agent=MAX_AGENTS, n_dir=MAX_DIRS, p="twin")]


def single(sizes, early, pointers, first, whitened=True):
    """Rows of a single-agent entry point: bad parameters, each size negative, the size that returns early, each
    required pointer, mean without inv_std and the reverse (whitened); `first`: its own rows, two faults at once
    among them."""
    rows = list(BAD_PARAMS)
    rows += [({s: -1}, SIZE) for s in sizes]
    rows += [({early: 0}, OK)]
    rows += [({q: None}, NULL) for q in pointers]
    return rows + (MEAN_XOR if whitened else []) + first


def multi(pointers, threads_code_with_null_pointer, first):
    """Rows of a multi-agent entry point: there is no early return, n_agent and n_dir start at 1."""
    rows = list(BAD_PARAMS)
    rows += [({s: v}, SIZE) for s in ("n_agent", "n_dir") for v in (0, -1)] + [(dict(H=-1), SIZE)]
    rows += [(dict(n_agent=MAX_AGENTS + 1), SIZE), (dict(n_dir=MAX_DIRS + 1), SIZE)]
    rows += [(t, SIZE) for t in TOO_MANY_THREADS]
    rows += [({q: None}, NULL) for q in pointers]
    rows += [(dict(TOO_MANY_THREADS[0], **{pointers[0]: None}), threads_code_with_null_pointer)]
    return rows + first


ROWS = {
    "sw_rollout_f64": single(
        ["n_roll", "H"], "n_roll", ["policies", "returns"],
        [(dict(H=-1, policies=None), SIZE), (dict(n_roll=0, H=-1), SIZE), (dict(n_roll=0, policies=None), OK),
         (dict(n_roll=0, mean=P), OK), (dict(p="n9", n_roll=-1), SEGMENTS), (dict(p="null", n_roll=-1), NULL),
         (dict(policies=None, mean=P), NULL)]),
    "sw_ars_rollouts_f64": single(
        ["dir_begin", "n_dir", "H"], "n_dir", ["policy", "deltas", "returns"],
        [(dict(n_dir=-1, deltas=None), SIZE), (dict(H=-1, policy=None), SIZE), (dict(n_dir=0, H=-1), SIZE),
         (dict(n_dir=0, deltas=None), OK), (dict(n_dir=0, dir_begin=-1), SIZE), (dict(p="n9", n_dir=-1), SEGMENTS),
         (dict(p="bad_l", deltas=None), PARAM)]),
    "sw_ars_gate_f64": single(
        ["dir_begin", "n_dir", "H"], "n_dir", ["policy", "deltas", "admit"],
        [(dict(n_dir=-1, admit=None), SIZE), (dict(H=-1, policy=None), SIZE), (dict(n_dir=0, H=-1), SIZE),
         (dict(n_dir=0, admit=None), OK), (dict(n_dir=0, mean=P), OK), (dict(p="n9", n_dir=-1), SEGMENTS),
         (dict(returns=None, admit=None), NULL), (dict(sim_thresh=NAN, admit=None), NULL)]),
    "sw_safe_rollouts_f64": single(
        ["n_roll", "H"], "n_roll", ["policies", "returns"],
        [(dict(sim="null"), NULL), (dict(sim="n9"), SEGMENTS), (dict(sim="bad_l"), PARAM), (dict(sim="n4"), SEGMENTS),
         (dict(p="n4"), SEGMENTS), (dict(p="n9", sim="null"), SEGMENTS), (dict(p="bad_l", sim="n9"), PARAM),
         (dict(sim="n4", n_roll=-1), SEGMENTS), (dict(sim="bad_l", p="n4"), PARAM),
         (dict(cost_kind=2), SIZE), (dict(cost_kind=-1), SIZE), (dict(cost_index=8), SIZE),
         (dict(cost_index=-1), SIZE), (dict(p="n4", sim="n4", cost_index=10), SIZE),
         (dict(sim_thresh=NAN), PARAM), (dict(real_thresh=NAN), PARAM),
         # the maximum |thetadot| cost has no index to check
         (dict(cost_kind=1, cost_index=8, policies=None), NULL),
         (dict(n_roll=-1, policies=None), SIZE), (dict(cost_kind=2, policies=None), SIZE),
         (dict(cost_index=8, returns=None), SIZE), (dict(sim_thresh=NAN, policies=None), PARAM),
         (dict(cost_kind=2, sim_thresh=NAN), SIZE), (dict(H=-1, real_thresh=NAN), SIZE),
         (dict(n_roll=0, cost_kind=2), SIZE), (dict(n_roll=0, cost_index=8), SIZE), (dict(n_roll=0, sim_thresh=NAN), PARAM),
         (dict(n_roll=0, policies=None), OK), (dict(n_roll=0, H=-1), SIZE)],
        whitened=False),
    "sw_ars_rollouts_multi_f64": multi(
        ["policy", "deltas", "returns"], NULL,
        MEAN_XOR + [(dict(n_agent=0, policy=None), SIZE), (dict(n_dir=0, deltas=None), SIZE),
                    (dict(H=-1, returns=None), SIZE), (dict(H=-1, mean=P), SIZE),
                    # the agent and direction limits and the thread count come behind the pointers
                    (dict(n_agent=MAX_AGENTS + 1, policy=None), NULL), (dict(n_dir=MAX_DIRS + 1, returns=None), NULL),
                    (dict(n_agent=MAX_AGENTS + 1, mean=P), NULL), (dict(TOO_MANY_THREADS[0], inv_std=P), NULL),
                    (dict(n_agent=MAX_AGENTS + 1, n_dir=0, policy=None), SIZE),
                    (dict(p="n9", n_agent=0), SEGMENTS)]),
    "sw_ars_gate_multi_f64": multi(
        ["policy", "deltas", "sim", "sim_thresh", "admit", "returns"], SIZE,
        MEAN_XOR + [(dict(n_agent=0, policy=None), SIZE), (dict(H=-1, admit=None), SIZE),
                    # every size check, the thread count included, comes before any pointer
                    (dict(n_agent=MAX_AGENTS + 1, policy=None), SIZE), (dict(n_dir=MAX_DIRS + 1, sim=None), SIZE),
                    (dict(TOO_MANY_THREADS[1], returns=None), SIZE), (dict(TOO_MANY_THREADS[0], mean=P), SIZE),
                    (dict(p="n9", n_agent=0), SEGMENTS), (dict(p="null", policy=None), NULL)]),
    "sw_ars_rollouts_multi_counted_f64": multi(
        ["count", "policy", "deltas", "returns"], SIZE,
        MEAN_XOR + [(dict(n_agent=0, count=None), SIZE), (dict(H=-1, policy=None), SIZE),
                    (dict(n_agent=MAX_AGENTS + 1, count=None), SIZE), (dict(n_dir=MAX_DIRS + 1, returns=None), SIZE),
                    (dict(TOO_MANY_THREADS[1], deltas=None), SIZE), (dict(TOO_MANY_THREADS[0], inv_std=P), SIZE),
                    (dict(p="n9", n_agent=0), SEGMENTS)]),
    "sw_safe_ars_rollouts_multi_f64": multi(
        ["policy", "deltas", "gated", "sim", "sim_thresh", "real_thresh", "returns"], NULL,
        [(dict(cost_kind=2), SIZE), (dict(cost_kind=-1), SIZE), (dict(cost_index=8), SIZE), (dict(cost_index=-1), SIZE),
         (dict(p="n4", cost_index=10), SIZE), (dict(cost_kind=1, cost_index=8, policy=None), NULL),
         (dict(n_agent=0, policy=None), SIZE), (dict(H=-1, gated=None), SIZE),
         (dict(n_agent=MAX_AGENTS + 1, policy=None), SIZE), (dict(n_dir=MAX_DIRS + 1, returns=None), SIZE),
         # the cost arguments come before the pointers, the thread count behind them
         (dict(cost_kind=2, policy=None), SIZE), (dict(cost_index=8, sim=None), SIZE),
         (dict(TOO_MANY_THREADS[1], returns=None), NULL), (dict(TOO_MANY_THREADS[0], cost_trace=P), SIZE),
         (dict(TOO_MANY_THREADS[0], cost_trace=P, real_thresh=None), NULL),
         (dict(TOO_MANY_THREADS[0], cost_kind=2), SIZE), (dict(p="n9", cost_kind=2), SEGMENTS)]),
}

CASES = [(entry, k, over, code) for entry, rows in ROWS.items() for k, (over, code) in enumerate(rows)]


def case_id(case):
    entry, k, over, code = case
    what = ",".join(f"{a}={'nan' if v != v else 'NULL' if v is None else 'ptr' if v is P else v}"
                    for a, v in over.items())
    return f"{entry[3:-4]}-{k}-{what}"


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    return swimmer_amd


def test_the_table_covers_the_eight_entry_points_and_no_row_expects_a_launch():
    assert set(ROWS) == set(SIGNATURES) and len(ROWS) == 8
    for entry, rows in ROWS.items():
        names = [a for a, _ in SIGNATURES[entry]]
        for over, code in rows:
            assert over and set(over) <= set(names), (entry, over)
            assert code in (OK, NULL, SEGMENTS, SIZE, PARAM), (entry, over)    # never SW_ERR_LAUNCH


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_point_return_code(sw, case):
    entry, _, over, code = case
    lib = sw._lib.load()
    keep = []                    # the parameter structs live until the call returns
    args = []
    for name, value in SIGNATURES[entry]:
        value = over.get(name, value)
        if isinstance(value, str):                     # a parameter set by name
            if value == "null":
                value = None
            else:
                keep.append(sw.SwParams.make(**PARAMS[value]))
                value = ctypes.byref(keep[-1])
        args.append(value)
    assert getattr(lib, entry)(*args) == code, (entry, over)
