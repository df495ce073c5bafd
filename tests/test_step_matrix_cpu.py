"""The step matrix (tests/step_matrix_cases.py, tests/step_reference.py) without a GPU.

 * COVERAGE.  INSTANTIATIONS has 115 entries; they are, name for name, the kernels of csrc/swimmer_step.hip in the
   built library's code object, and the parametrisation of tests/test_step_matrix_gpu.py launches each.
 * THE REFERENCE IS THE REFERENCE.  The long-double restatement reproduces tests/golden/steps.npz (the reference's
   own outputs) inside its bounds and the twin's recorded known answers to the digits printed; its sines and cosines
   of the edge angles agree with 40-digit values to 2^-62.  R_oracle, the fp64 oracle's worst ratio under K = 1 over
   every case, is measured here, and K_MEASURED must be 4 R_oracle rounded up to a power of two.
 * THE BOUNDS ARE SHARP.  For every case max C / max |ref| <= 256, and in the calm regime bound_step <= 1e-13
   max(1, |state|).  A condition on the cases, not a measurement of a kernel.
 * THE CASES CAN CATCH WHAT THEY ARE FOR.  On the fp64 oracle: k (1 + 1e-12), and l likewise, push an environment
   over its bound at every n; a swapped direction shows in every reward; the angle moved with the other thetadot
   (the new one in the Gym model, the old one in the twin) shows in every environment; a distance taken without the
   Gdot components shows in every residual case of the `noise` store and, where a moved transition is inside, of the
   `moved` store (in the `rounded` store the distance itself is at rounding level: nothing of it can show).
"""
import json
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, PARAM_SETS, ROOT, observed
from test_loop_placement import LIB, LLVM, _disassemble

import step_matrix_cases as mc
import step_reference as sr
from step_reference import LD, Ref

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")
CASES = [(model, n, pi) for model in mc.MODELS for n in mc.NS for pi in range(len(mc.param_sets(model)))]


def test_the_list_has_115_entries_and_the_gpu_test_launches_each():
    assert len(mc.INSTANTIATIONS) == 115 and len({i.symbol for i in mc.INSTANTIATIONS}) == 115
    assert [len(mc.find(k)) for k in mc.KERNEL_NAMES] == list(mc.COUNTS) and sum(mc.COUNTS) == 115
    reached = mc.reached_by()
    assert set().union(*map(set, reached.values())) == set(mc.INSTANTIATIONS)
    source = open(os.path.join(ROOT, "tests", "test_step_matrix_gpu.py")).read()
    for name in reached:
        assert re.search(rf"^def {name}\(", source, flags=re.M), name


@needs_tools
def test_every_compiled_instantiation_is_listed_once():
    pattern = re.compile("(?:" + "|".join(f"_GLOBAL__N_1{len(k)}{k}[IE]" for k in mc.KERNEL_NAMES) + ")")
    symbols = sorted({l.split("<", 1)[1][:-2] for l in _disassemble()
                      if l.startswith("0000") and l.endswith(">:") and pattern.search(l)})
    assert len(symbols) == 115, (len(symbols), symbols)
    for s in symbols:
        named_by = [i.symbol for i in mc.INSTANTIATIONS if i.symbol in s]
        assert len(named_by) == 1, (s, named_by)
    for i in mc.INSTANTIATIONS:
        assert sum(i.symbol in s for s in symbols) == 1, (i, "is not in the library")


def test_the_nt_sizes_cross_the_streaming_threshold():
    for n in mc.NS:
        T, per = mc.nt_transitions(n), 8 * (2 * (2 * n + 2) + n)
        assert T % mc.NT_PATTERN == mc.NT_TAIL and T * per > mc.STREAM_BYTES >= (T - mc.NT_PATTERN) * per
    assert mc.nt_transitions(2) == 2397697 and mc.nt_transitions(8) == 763393


def test_the_edge_set():
    e = mc.EDGE_ANGLES
    assert (np.abs(e) < mc.ANGLE_LIMIT).all() and np.abs(e).max() == np.nextafter(3e9, 0)
    assert {0.0, 5e-324, 1e-300, float(np.float64(np.pi / 2)), float(np.float64(-np.pi))} <= set(e.tolist())
    assert np.signbit(e[e == 0]).any() and not np.signbit(e[e == 0]).all()
    # every (model, n): the edge environments of the parameter sets together hold every edge angle
    for model in mc.MODELS:
        seen = np.concatenate([mc.case(model, 2, pi)["unique"][0][-mc.UNIQUE[model][1]:, 2::2].ravel()
                               for pi in range(len(mc.param_sets(model)))])
        assert set(e.tolist()) <= set(seen.tolist())
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    s, c = np.sin(LD(1) * e), np.cos(LD(1) * e)
    worst = 0.0
    for x, si, ci in zip(e, s, c):
        xs = mpmath.mpf(float(x))
        # a long double is the sum of its two float64 halves, exactly
        for got, want in ((si, mpmath.sin(xs)), (ci, mpmath.cos(xs))):
            hi = float(got)
            lo = float(got - LD(hi))
            worst = max(worst, abs(float(mpmath.mpf(hi) + mpmath.mpf(lo) - want)))
    assert worst <= 2.0 ** -62, worst


def test_the_reference_reproduces_the_recorded_outputs():
    """tests/golden/steps.npz holds the reference's own fp64 outputs (NumPy, LAPACK's solve): another fp64 evaluation
    of the same statements, held to the bounds the kernels are held to."""
    g = np.load(os.path.join(GOLDEN, "steps.npz"))
    worst = {}
    for key in sorted({k.rsplit("_", 1)[0] for k in g.files}):
        n, pset = int(key[1]), key.split("_", 1)[1]
        l, m, k, h = PARAM_SETS[pset]
        ref = sr.step_ref("gym", l, m, k, h, g[key + "_dir"], g[key + "_state"], g[key + "_action"],
                          K=mc.K_MEASURED["gym"])
        got = np.concatenate([g[key + "_gdd"], g[key + "_tdd"]], axis=1)
        worst[key] = (sr.ratio(got, ref["accel"]), sr.ratio(g[key + "_next"], ref["next"]),
                      sr.ratio(g[key + "_reward"], ref["reward"]))
        assert max(worst[key]) <= 1.0, (key, worst[key])
        # and absolutely: the recorded next states are doubles next to the long-double ones
        assert np.abs(g[key + "_next"] - ref["next"].value.astype(np.float64)).max() <= 1e-14
    print("golden steps, worst ratio (accel, next, reward):", np.max(list(worst.values()), axis=0))


def test_the_twin_reference_reproduces_the_known_answers():
    from test_twin import KAT_GDD, KAT_H, KAT_NEXT, KAT_STATE, KAT_TDD, KAT_TORQUE, sig6
    with open(os.path.join(GOLDEN, "twin_kat.json")) as f:
        rec = json.load(f)
    st, ac = np.array([rec["state"]]), np.array([rec["torque"]])
    assert rec["state"] == KAT_STATE and rec["torque"] == KAT_TORQUE
    ref = sr.step_ref("twin", rec["l_i"], rec["m_i"], rec["k"], KAT_H, (1.0, 0.0), st, ac)
    acc = ref["accel"].value[0].astype(np.float64)
    assert sig6(acc[:2], KAT_GDD) and sig6(acc[2:], KAT_TDD)
    assert sig6(acc[:2], rec["G_dotdot"]) and sig6(acc[2:], rec["angle_accelerations"])
    assert sig6(ref["next"].value[0].astype(np.float64), KAT_NEXT)


def test_r_oracle_fixes_k():
    r_oracle = {m: mc.r_oracle(m) for m in mc.MODELS}
    figures = {"R_oracle": r_oracle, "K": {m: sr.k_from(r) for m, r in r_oracle.items()}}
    observed("step_matrix_cpu", figures)
    assert figures["K"] == mc.K_MEASURED, figures
    # with that K the oracle is inside every bound, by the factor 4 in the accelerations
    for model, n, pi in CASES:
        acc, nxt, rew = mc.oracle_ratios(model, n, pi)
        assert acc.max() <= 0.25 * mc.K_MEASURED[model] and nxt <= 1.0 and rew <= 1.0, \
            (model, n, pi, acc.max(), nxt, rew)
    recorded = os.path.join(ROOT, "profiles", "step_matrix_observed.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            rec = json.load(f)
        assert rec["K"] == mc.K_MEASURED and all(abs(rec["R_oracle"][m] - r_oracle[m]) <= 0.02 * r_oracle[m]
                                                 for m in mc.MODELS), (rec["R_oracle"], r_oracle)


@pytest.mark.parametrize("model,n,pi", CASES)
def test_the_bounds_are_sharp(model, n, pi):
    c, ref = mc.case(model, n, pi), mc.reference(model, n, pi)
    assert np.isfinite(ref["sharp"]).all() and ref["sharp"].max() <= 256, ref["sharp"].max()
    calm = c["regime"] == mc.REGIMES.index("calm")
    assert calm.sum() >= 3 * mc.UNIQUE[model][0] if model == "twin" else calm.sum() == mc.UNIQUE[model][0]
    room = ref["next"].bound[calm] / np.maximum(1.0, np.abs(c["state"][calm]))
    assert room.max() <= 1e-13, room.max()
    assert (ref["reward"].bound[calm] <= 1e-13).all()
    for key in ("accel", "next", "reward"):
        assert np.isfinite(ref[key].value.astype(np.float64)).all() and (ref[key].bound > 0).all()


def _over(got, ref):
    """[E]: the worst ratio of every environment."""
    got = np.asarray(got).reshape(len(got), -1)
    diff = np.abs(LD(1) * got - ref.value.reshape(got.shape)).astype(np.float64)
    return (diff / np.broadcast_to(ref.bound.reshape(len(got), -1), diff.shape)).max(axis=1)


@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("n", mc.NS)
def test_a_wrong_parameter_goes_over_a_bound(model, n):
    for scale in (dict(scale_k=1.0 + 1e-12), dict(scale_l=1.0 + 1e-12)):
        over = 0
        for pi in range(len(mc.param_sets(model))):
            acc, nxt, _ = mc.oracle_outputs(model, n, pi, **scale)
            ref = mc.reference(model, n, pi)
            over += int((np.maximum(_over(acc, ref["accel"]), _over(nxt, ref["next"])) > 1.0).sum())
        assert over >= 1, (model, n, scale)


@pytest.mark.parametrize("model,n,pi", CASES)
def test_a_swapped_direction_and_the_other_thetadot_show(model, n, pi):
    c, ref = mc.case(model, n, pi), mc.reference(model, n, pi)
    _, _, rew = mc.oracle_outputs(model, n, pi, direction=c["direction"][::-1])
    assert (_over(rew, ref["reward"]) > 1.0).all()
    acc, nxt, _ = mc.oracle_outputs(model, n, pi)
    wrong, _ = sr.euler("gym" if model == "twin" else "twin", c["h"], c["direction"], c["state"], acc, xp=np.float64)
    assert np.array_equal(wrong[:, 3::2], nxt[:, 3::2])
    assert (_over(wrong[:, 2::2], Ref(ref["next"].value[:, 2::2], ref["next"].bound[:, 2::2])) > 1.0).all()


@pytest.mark.parametrize("n", mc.NS)
def test_a_distance_without_gdot_shows(n):
    _, nxt, _ = mc.oracle_outputs("gym", n, 1)
    tr = mc.transitions(n, 1)
    for store in ("noise", "moved"):
        for T in mc.RES_SIZES:
            if store == "moved" and T < 255:
                continue                                     # no moved transition inside
            ref = mc.residual_reference(n, 1, store, T)
            diff = (mc.tile(nxt, T) - tr["stores"][store][:T])[:, 2:]
            dist = np.concatenate([np.sqrt((diff * diff).sum(axis=1)), np.zeros(sr.blocks(T) * sr.BLOCK - T)])
            wrong = dist.reshape(-1, sr.BLOCK).sum(axis=1)
            assert sr.ratio(wrong, ref) > 1.0, (store, T)
            right = np.sqrt(((mc.tile(nxt, T) - tr["stores"][store][:T]) ** 2).sum(axis=1))
            right = np.concatenate([right, np.zeros(sr.blocks(T) * sr.BLOCK - T)]).reshape(-1, sr.BLOCK).sum(axis=1)
            assert sr.ratio(right, ref) <= 1.0, (store, T)


@pytest.mark.parametrize("n", (2, 5, 8))
def test_the_oracle_is_inside_the_residual_and_normal_bounds(n):
    """The fp64 oracle's next states, reduced in plain float64 NumPy (another order of summation), are inside the
    residual bounds of every store and size and inside the propagated bounds of the normal equations."""
    pi = 1
    _, nxt, _ = mc.oracle_outputs("gym", n, pi)
    tr = mc.transitions(n, pi)
    for store in mc.STORES:
        for T in mc.RES_SIZES:
            d = np.sqrt(((mc.tile(nxt, T) - tr["stores"][store][:T]) ** 2).sum(axis=1))
            got = np.concatenate([d, np.zeros(sr.blocks(T) * sr.BLOCK - T)]).reshape(-1, sr.BLOCK).sum(axis=1)
            ref = mc.residual_reference(n, pi, store, T)
            assert sr.ratio(got, ref) <= 1.0, (store, T, sr.ratio(got, ref))
            assert sr.ratio(got.sum(), sr.row_total(ref)) <= 1.0
    import oracle
    c, tr = mc.case("gym", n, pi), mc.set_transitions(n, pi)
    points, inv = mc.normal_points(n, pi, 7)
    for s in (1, 4):
        b0 = int(mc.set_begin()[s])
        sl = slice(b0, b0 + mc.SET_LENGTHS[s])
        got_r = [oracle.step_batch(oracle.OracleParams.make(n, l, m, k, c["h"], c["direction"]), tr["state"][sl],
                                   tr["action"][sl])[0] - tr["stored"][sl] for l, m, k in points[s]]
        J = [(got_r[1 + 2 * i] - got_r[2 + 2 * i]) * inv[s][i] for i in range(3)]
        got = [np.sum(got_r[0] * got_r[0])] + [np.sum(a * b) for a in J for b in J] + [np.sum(a * got_r[0]) for a in J]
        ref = mc.normal_reference(n, pi, s, 7)
        assert np.isfinite(ref.value.astype(np.float64)).all() and (ref.bound > 0).all()
        assert sr.ratio(np.array(got), ref) <= 1.0, (s, sr.ratio(np.array(got), ref))
        assert sr.ratio(np.array(got[:1]), mc.normal_reference(n, pi, s, 1)) <= 1.0
        # the bound decides something: r.r to eight digits, every other sum far below the largest of its kind
        assert ref.bound[0] <= 1e-8 * float(ref.value[0]), ref.bound
        assert ref.bound[1:10].max() <= 1e-3 * float(np.abs(ref.value[1:10]).max()), ref.bound
        assert ref.bound[10:].max() <= 1e-3 * float(np.abs(ref.value[10:]).max()), ref.bound


def test_the_row_sum_restatement():
    rs = np.random.RandomState(5)
    for nb in (1, 3, 64, 65, 200):
        row = rs.uniform(0.0, 1.0, nb)
        got = sr.row_sum_fixed_order(row)
        assert abs(got - float(np.sum(LD(1) * row))) <= sr.gamma(nb + 16) * row.sum()
    # the order is the documented one: 2^53 in lane 0's first entry absorbs a 1.0 added to it directly (entry 64),
    # not one that arrives through the tree in a pair (entries 1 and 2 meet in lane 1 ... only after lane sums)
    row = np.zeros(65)
    row[0], row[64] = 2.0 ** 53, 1.0
    assert sr.row_sum_fixed_order(row) == 2.0 ** 53
    row = np.zeros(65)
    row[0], row[32], row[16] = 2.0 ** 53, 1.0, 1.0       # lane 32 joins first (absorbed), then lane 16 (absorbed)
    assert sr.row_sum_fixed_order(row) == 2.0 ** 53
    row[32], row[16], row[48] = 0.0, 1.0, 1.0            # 16 and 48 meet first: 2.0 survives
    assert sr.row_sum_fixed_order(row) == 2.0 ** 53 + 2.0
