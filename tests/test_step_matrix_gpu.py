"""Every kernel of the step family (csrc/swimmer_step.hip) against the long-double reference of
tests/step_reference.py, at the cases of tests/step_matrix_cases.py (whose 115 INSTANTIATIONS
tests/test_step_matrix_cpu.py compares with the library's code object).

 * step, accel, reset, per (n, model): every parameter set, every batch size and regime inside the bounds; status 0
   where it should be and the status cases exactly as the header defines them; every output in the middle of a buffer
   whose 64 guard entries in front and behind stay untouched; in place (out = state) and through StepPlan.launch()
   the bits of the out-of-place call; reward / status NULL in all four combinations; reset the oracle's reset state.
 * NT step forms: one child process with SWIMMER_STEP_NT=1 (read once per process) reruns the Gym step cases; the
   parent holds its outputs bit for bit to the plain forms', which are inside the bounds.
 * env1: all 28, bit for bit the batched kernel on one environment of every regime, status cases included.
 * residual, single: the three stores and five sizes inside the bounds, twice with equal bits; the NT forms on a batch
   tiled on the device from a 1024-transition pattern beyond 256 MiB of traffic: block b has the bits of block b mod 4
   of the plain launch on the pattern, the last three those of the plain launch on its first 513 transitions.
 * population (plain and NT) and sets: bit for bit the single kernel per candidate; value is the row sum in the
   documented order, restated in NumPy; entries behind a set's last block untouched.
 * normal equations, n_point 1 and 7: inside the propagated bounds, the lower triangle the upper one's bits, the
   inactive set untouched.

The worst ratio of every kernel and n, and where it occurred, go to observed("step_matrix", ...) with R_oracle and K;
profiles/step_matrix_observed.json holds those of the first run.  A ratio above 1 is a failure: it is answered by
finding the operation responsible, never by a larger K.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import observed

import step_matrix_cases as mc
import step_reference as sr
from step_reference import Ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIGURES, LAUNCHED, RAN = {}, set(), set()
NT_OUT = "STEP_MATRIX_NT_OUT"            # set in the child: where it writes its outputs


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


def soa(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).T), device=DEV, dtype=dtype)


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV, dtype=dtype)


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = host(a) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


def same_nan(a, b):
    """Equal bits, but a NaN for a NaN whatever its sign and payload (two kernels may order an operation on a NaN
    input differently)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.array_equal(bits(np.where(nan, 0.0, a)), bits(np.where(nan, 0.0, b))))


def params(sw, model, n, l, m, k, h, direction):
    return sw.SwParams.make(n, l, m, k, h, direction, flags=sw._lib.FLAG_MODEL_TWIN if model == "twin" else 0)


def case_params(sw, c):
    return params(sw, c["model"], c["n"], c["l"], c["m"], c["k"], c["h"], c["direction"])


def guarded(shape, dtype=torch.float64):
    """(buffer, view): a contiguous tensor of `shape` in the middle of a buffer with GUARD poisoned entries in front
    and behind."""
    fill = mc.POISON if dtype == torch.float64 else -77
    numel = int(np.prod(shape))
    buf = torch.full((2 * mc.GUARD + numel,), fill, dtype=dtype, device=DEV)
    return buf, buf[mc.GUARD:mc.GUARD + numel].view(shape)


def intact(buf):
    b = host(buf)
    fill = mc.POISON if b.dtype == np.float64 else -77
    return bool((b[:mc.GUARD] == fill).all() and (b[-mc.GUARD:] == fill).all())


def note(kernel, n, value, where):
    key = f"{kernel} n={n}"
    if key not in FIGURES or value > FIGURES[key]["ratio"]:
        FIGURES[key] = {"ratio": float(value), "where": str(where)}


def launched(test, name, **kw):
    found = mc.find(name, **kw)
    assert found and set(found) <= set(mc.reached_by()[test]), (test, name, kw)
    LAUNCHED.update(found)
    RAN.add(test)


def run_step(sw, p, st, ac, reward=True, status=True):
    """sw_step_f64 into guarded buffers -> (next [d, B], reward [B] or None, status [B] or None) as NumPy arrays;
    reward / status False: NULL."""
    d, B = st.shape
    ob, out = guarded((d, B))
    rb, rew = guarded((B,)) if reward else (None, None)
    sb, sta = guarded((B,), torch.int32) if status else (None, None)
    sw._lib.check(sw._lib.load().sw_step_f64(ctypes.byref(p), B, sw._lib.ptr(st), sw._lib.ptr(ac), sw._lib.ptr(out),
                                             sw._lib.ptr(rew), sw._lib.ptr(sta), sw._lib.stream_ptr()), "sw_step_f64")
    torch.cuda.synchronize()
    assert intact(ob) and (rb is None or intact(rb)) and (sb is None or intact(sb))
    return host(out), None if rew is None else host(rew), None if sta is None else host(sta)


def run_accel(sw, p, st, ac):
    d, B = st.shape
    gb, gdd = guarded((2, B))
    tb, tdd = guarded((p.n, B))
    sw._lib.check(sw._lib.load().sw_accel_f64(ctypes.byref(p), B, sw._lib.ptr(st), sw._lib.ptr(ac), sw._lib.ptr(gdd),
                                              sw._lib.ptr(tdd), sw._lib.stream_ptr()), "sw_accel_f64")
    torch.cuda.synchronize()
    assert intact(gb) and intact(tb)
    return np.concatenate([host(gdd), host(tdd)])          # [n + 2, B]


def head(ref, B, T=False):
    v, b = ref.value[:B], ref.bound[:B]
    return Ref(v.T, b.T) if T else Ref(v, b)


@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("n", mc.NS)
def test_step_accel_within_bounds(sw, n, model):
    twin = model == "twin"
    launched("test_step_accel_within_bounds", "step_kernel", n=n, twin=twin, nt=None)
    launched("test_step_accel_within_bounds", "accel_kernel", n=n, twin=twin)
    for pi in range(len(mc.param_sets(model))):
        c, ref = mc.case(model, n, pi), mc.reference(model, n, pi)
        p = case_params(sw, c)
        for B in mc.SIZES:
            st, ac = soa(c["state"][:B]), soa(c["action"][:B])
            nxt, rew, sta = run_step(sw, p, st, ac)
            acc = run_accel(sw, p, st, ac)
            assert not sta.any(), (pi, B, np.flatnonzero(sta))
            for kernel, got, r in (("step_kernel next", nxt, head(ref["next"], B, True)),
                                   ("step_kernel reward", rew, head(ref["reward"], B)),
                                   ("accel_kernel", acc, head(ref["accel"], B, True))):
                q = sr.ratio(got, r)
                note(f"{kernel} {model}", n, q, f"set {pi}, {B} environments")
                assert q <= 1.0, (kernel, pi, B, q)
            # in place, and pre-bound
            st2 = st.clone()
            out2, rew2 = sw.kernels.step(p, st2, ac, out=st2)
            assert out2 is st2 and same(st2, nxt) and same(rew2, rew)
            out3, rew3 = torch.empty_like(st), torch.empty(B, dtype=torch.float64, device=DEV)
            sta3 = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            sw.kernels.StepPlan(p, st, ac, out3, rew3, sta3).launch()
            assert same(out3, nxt) and same(rew3, rew) and not host(sta3).any()
        # reward / status NULL in every combination, at a size with a partial workgroup
        B = 257
        st, ac = soa(c["state"][:B]), soa(c["action"][:B])
        full = run_step(sw, p, st, ac)
        for reward, status in ((True, False), (False, True), (False, False)):
            got = run_step(sw, p, st, ac, reward, status)
            assert same(got[0], full[0]) and (not reward or same(got[1], full[1])) \
                and (not status or same(got[2], full[2]))
    # the status cases, on the first parameter set
    c, ref = mc.case(model, n, 0), mc.reference(model, n, 0)
    p, B = case_params(sw, c), mc.STATUS_N_ENV
    plain = run_step(sw, p, soa(c["state"][:B]), soa(c["action"][:B]))
    plain_acc = run_accel(sw, p, soa(c["state"][:B]), soa(c["action"][:B]))
    others = np.setdiff1d(np.arange(B), mc.STATUS_LANES)
    for kind, (name, _, _, must, must_not) in enumerate(mc.STATUS_KINDS):
        st, ac, lanes = mc.status_case(model, n, kind)
        st, ac = soa(st), soa(ac)
        nxt, rew, sta = run_step(sw, p, st, ac)
        acc = run_accel(sw, p, st, ac)
        lanes = list(lanes)
        assert ((sta[lanes] & must) == must).all() and not (sta[lanes] & must_not).any(), (name, sta[lanes])
        assert not np.isfinite(nxt[:, lanes]).all(axis=0).any(), name
        if must & mc.STATUS_RANGE:
            assert np.isnan(nxt[:, lanes]).all() and np.isnan(rew[lanes]).all() and np.isnan(acc[:, lanes]).all(), name
        # the neighbours: status 0 and the bits of the batch without the fault, which is inside its bounds
        assert not sta[others].any(), (name, np.flatnonzero(sta))
        assert same(nxt[:, others], plain[0][:, others]) and same(rew[others], plain[1][others])
        assert same(acc[:, others], plain_acc[:, others])
        for reward, status in ((True, False), (False, True), (False, False)):
            got = run_step(sw, p, st, ac, reward, status)
            assert same(got[0], nxt) and (not reward or same(got[1], rew)) and (not status or same(got[2], sta))
    assert sr.ratio(plain[0], head(ref["next"], B, True)) <= 1.0


@pytest.mark.parametrize("model", mc.MODELS)
def test_reset(sw, model):
    launched("test_reset", "reset_kernel")
    for n in mc.NS:
        p = params(sw, model, n, 1.0, 1.0, 10.0, 1e-3, (1.0, 0.0))
        for B in mc.RESET_SIZES:
            buf, out = guarded((p.d, B))
            assert sw.kernels.reset(p, B, device=DEV, out=out) is out
            torch.cuda.synchronize()
            assert intact(buf) and same(host(out).T, mc.reset_state(model, n, B)), (n, B)


def gym_step_outputs(sw):
    """{(n, pi, B): (next, reward, status)} of the Gym step cases through sw_step_f64, whatever form it takes."""
    out = {}
    for n in mc.NS:
        for pi in range(len(mc.param_sets("gym"))):
            c = mc.case("gym", n, pi)
            p = case_params(sw, c)
            for B in mc.SIZES:
                out[n, pi, B] = run_step(sw, p, soa(c["state"][:B]), soa(c["action"][:B]))
    return out


def test_nt_step_forms_in_a_child_process(sw, tmp_path):
    """step_kernel<N, false, true> takes batches this small only with SWIMMER_STEP_NT=1, which the library reads once
    per process: the Gym step cases once more in a fresh child, whose outputs must be the plain forms' bits (which
    test_step_accel_within_bounds holds to the bounds)."""
    if os.environ.get(NT_OUT):            # the child
        assert os.environ.get("SWIMMER_STEP_NT") == "1"
        got = gym_step_outputs(sw)
        np.savez(os.environ[NT_OUT],
                 **{f"{n}_{pi}_{B}_{j}": a for (n, pi, B), v in got.items() for j, a in enumerate(v)})
        return
    for n in mc.NS:
        launched("test_nt_step_forms_in_a_child_process", "step_kernel", n=n, nt="forced")
    assert os.environ.get("SWIMMER_STEP_NT") in (None, "", "0"), "the parent must run the plain forms"
    path = str(tmp_path / "nt_step.npz")
    env = dict(os.environ, SWIMMER_STEP_NT="1", **{NT_OUT: path})
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                          "-k", "test_nt_step_forms_in_a_child_process"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    child, plain = np.load(path), gym_step_outputs(sw)
    assert len(child.files) == 3 * len(plain)
    for (n, pi, B), v in plain.items():
        for j, a in enumerate(v):
            assert same(child[f"{n}_{pi}_{B}_{j}"], a), (n, pi, B, j)


@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("n", mc.NS)
def test_env1_is_the_batched_kernel(sw, n, model):
    for accel in (False, True):
        launched("test_env1_is_the_batched_kernel", "env1_kernel", n=n, twin=model == "twin", accel=accel)
    K = sw.kernels.SingleEnv
    d, m = 2 * n + 2, n - 1
    h = K()
    try:
        for pi in range(len(mc.param_sets(model))):
            c = mc.case(model, n, pi)
            p = case_params(sw, c)
            pick = [int(np.flatnonzero(c["regime"] == r)[0]) for r in range(len(mc.REGIMES))]
            batches = [(c["state"][pick], c["action"][pick])]
            if pi == 0:                                      # the status cases: lane 0 of each kind
                kinds = [mc.status_case(model, n, kind) for kind in range(len(mc.STATUS_KINDS))]
                batches.append((np.stack([s[0] for s, _, _ in kinds]), np.stack([a[0] for _, a, _ in kinds])))
            for st, ac in batches:
                nxt, rew, sta = run_step(sw, p, soa(st), soa(ac))
                acc = run_accel(sw, p, soa(st), soa(ac))
                for e in range(len(st)):
                    h.io[:] = mc.POISON
                    h.io[K.STATE:K.STATE + d], h.io[K.ACTION:K.ACTION + m] = st[e], ac[e]
                    got = h.step(p)
                    assert got == sta[e], (pi, e, got, sta[e])
                    assert same_nan(h.io[K.NEXT:K.NEXT + d], nxt[:, e]) and \
                        same_nan(h.io[K.REWARD:K.REWARD + 1], rew[e:e + 1]), (pi, e)
                    assert same(h.io[K.STATE:K.STATE + d].copy(), st[e])
                    h.accelerations(p)
                    assert same_nan(h.io[K.GDD:K.GDD + 2], acc[:2, e]) and \
                        same_nan(h.io[K.TDD:K.TDD + n], acc[2:, e]), (pi, e)
    finally:
        h.close()


def residual(sw, p, st, ac, stored):
    nb = sr.blocks(st.shape[1])
    buf, partial = guarded((nb,))
    assert sw.kernels.step_residual(p, st, ac, stored, partial=partial) is partial
    torch.cuda.synchronize()
    assert intact(buf)
    return host(partial)


def res_set(n):
    return n % len(mc.GYM_SETS)            # the parameter set the residual tests of n run on


@pytest.mark.parametrize("n", mc.NS)
def test_residual_single(sw, n):
    launched("test_residual_single", "step_residual_kernel", n=n, nt=None)
    pi = res_set(n)
    c, tr = mc.case("gym", n, pi), mc.transitions(n, pi)
    p = case_params(sw, c)
    for store in mc.STORES:
        for T in mc.RES_SIZES + (mc.RES_T,):
            st, ac, nx = soa(tr["state"][:T]), soa(tr["action"][:T]), soa(tr["stores"][store][:T])
            got = residual(sw, p, st, ac, nx)
            assert same(residual(sw, p, st, ac, nx), got)
            ref = mc.residual_reference(n, pi, store, T)
            q = sr.ratio(got, ref)
            note(f"step_residual_kernel {store}", n, q, f"{T} transitions")
            assert q <= 1.0, (store, T, q)
            assert sr.ratio(got.sum(), sr.row_total(ref)) <= 1.0


def tiled(n, pi):
    """The NT batch on the device: q copies of the 1024-transition pattern and its first 513 transitions."""
    tr = mc.transitions(n, pi)
    T = mc.nt_transitions(n)
    q = T // mc.NT_PATTERN

    def big(a):
        a = soa(a)
        return torch.cat([a.repeat(1, q), a[:, :mc.NT_TAIL]], dim=1).contiguous()
    return q, big(tr["state"]), big(tr["action"]), big(tr["stores"]["noise"])


@pytest.mark.parametrize("n", mc.NS)
def test_residual_nt_forms(sw, n):
    launched("test_residual_nt_forms", "step_residual_kernel", n=n, nt="size")
    launched("test_residual_nt_forms", "step_residual_pop_kernel", n=n, nt="size")
    launched("test_residual_nt_forms", "residual_rows_sum_kernel")
    pi = res_set(n)
    c, tr = mc.case("gym", n, pi), mc.transitions(n, pi)
    p = case_params(sw, c)
    q, st, ac, nx = tiled(n, pi)
    T = st.shape[1]
    assert T == mc.nt_transitions(n) and T * 8 * (2 * p.d + n) > mc.STREAM_BYTES
    plain4 = residual(sw, p, soa(tr["state"]), soa(tr["action"]), soa(tr["stores"]["noise"]))
    plain3 = residual(sw, p, soa(tr["state"][:mc.NT_TAIL]), soa(tr["action"][:mc.NT_TAIL]),
                      soa(tr["stores"]["noise"][:mc.NT_TAIL]))
    for plain, size in ((plain4, mc.RES_T), (plain3, mc.NT_TAIL)):      # the plain launches are inside their bounds
        assert sr.ratio(plain, mc.residual_reference(n, pi, "noise", size)) <= 1.0
    got = residual(sw, p, st, ac, nx)
    assert got.shape == (4 * q + 3,)
    assert same(got[:4 * q].reshape(q, 4), np.tile(plain4, (q, 1))) and same(got[4 * q:], plain3)
    # the population's NT form on the same batch: per candidate the single (NT) kernel's bits
    cand = mc.candidates(n, pi, mc.POP_CANDIDATES)
    value, partial, status = sw.kernels.step_residual_population(p, dev(cand), st, ac, nx)
    partial, value = host(partial), host(value)
    assert not host(status).any()
    for j, (l, m, k) in enumerate(cand):
        pj = params(sw, "gym", n, l, m, k, c["h"], c["direction"])
        assert same(residual(sw, pj, st, ac, nx), partial[j]), j
        assert same(np.array([sr.row_sum_fixed_order(partial[j])]), value[j:j + 1]), j


@pytest.mark.parametrize("n", mc.NS)
def test_residual_population(sw, n):
    launched("test_residual_population", "step_residual_pop_kernel", n=n, nt=None)
    launched("test_residual_population", "residual_rows_sum_kernel")
    pi = res_set(n)
    c, tr = mc.case("gym", n, pi), mc.transitions(n, pi)
    p = case_params(sw, c)
    cand = mc.candidates(n, pi, mc.POP_CANDIDATES)
    for store in mc.STORES:
        for T in (257, 1000):
            st, ac, nx = soa(tr["state"][:T]), soa(tr["action"][:T]), soa(tr["stores"][store][:T])
            pbuf, partial = guarded((len(cand), sr.blocks(T)))
            vbuf, value = guarded((len(cand),))
            sbuf, status = guarded((len(cand),), torch.int32)
            sw.kernels.step_residual_population(p, dev(cand), st, ac, nx, partial=partial, value=value, status=status)
            torch.cuda.synchronize()
            assert intact(pbuf) and intact(vbuf) and intact(sbuf) and not host(status).any()
            partial, value = host(partial), host(value)
            for j, (l, m, k) in enumerate(cand):
                pj = params(sw, "gym", n, l, m, k, c["h"], c["direction"])
                assert same(residual(sw, pj, st, ac, nx), partial[j]), (store, T, j)
                assert same(np.array([sr.row_sum_fixed_order(partial[j])]), value[j:j + 1]), (store, T, j)
            # candidate 0 is the set's own parameters: inside the single kernel's bounds
            assert sr.ratio(partial[0], mc.residual_reference(n, pi, store, T)) <= 1.0


@pytest.mark.parametrize("n", mc.NS)
def test_residual_sets(sw, n):
    launched("test_residual_sets", "step_residual_sets_kernel", n=n)
    launched("test_residual_sets", "residual_set_rows_sum_kernel")
    pi = res_set(n)
    c, tr = mc.case("gym", n, pi), mc.set_transitions(n, pi)
    p = case_params(sw, c)
    begin, longest = mc.set_begin(), max(mc.SET_LENGTHS)
    cand_set = np.array(mc.SET_OF_CANDIDATE, dtype=np.int32)
    cand = mc.candidates(n, pi, len(cand_set))
    st, ac, nx = soa(tr["state"]), soa(tr["action"]), soa(tr["stored"])
    nb = sr.blocks(longest)
    pbuf, partial = guarded((len(cand), nb))
    vbuf, value = guarded((len(cand),))
    sbuf, status = guarded((len(cand),), torch.int32)
    sw.kernels.step_residual_sets(p, dev(begin, torch.int64), longest, dev(cand), dev(cand_set, torch.int32), st, ac,
                                  nx, partial=partial, value=value, status=status)
    torch.cuda.synchronize()
    assert intact(pbuf) and intact(vbuf) and intact(sbuf) and not host(status).any()
    partial, value = host(partial), host(value)
    assert set(cand_set.tolist()) == {0, 1, 2, 4}            # set 3 has no candidate
    for j, (l, m, k) in enumerate(cand):
        s = int(cand_set[j])
        sl = slice(int(begin[s]), int(begin[s + 1]))
        pj = params(sw, "gym", n, l, m, k, c["h"], c["direction"])
        alone = residual(sw, pj, soa(tr["state"][sl]), soa(tr["action"][sl]), soa(tr["stored"][sl]))
        assert same(alone, partial[j, :len(alone)]), j
        assert (partial[j, len(alone):] == mc.POISON).all(), j          # behind the set's last block: untouched
        assert same(np.array([sr.row_sum_fixed_order(alone)]), value[j:j + 1]), j


@pytest.mark.parametrize("n_point", mc.N_POINTS)
@pytest.mark.parametrize("n", mc.NS)
def test_residual_normal_sets(sw, n, n_point):
    launched("test_residual_normal_sets", "step_residual_normal_sets_kernel", n=n, n_point=n_point)
    launched("test_residual_normal_sets", "residual_set_rows_sum_kernel")
    pi = res_set(n)
    c, tr = mc.case("gym", n, pi), mc.set_transitions(n, pi)
    p = case_params(sw, c)
    begin, longest, n_set = mc.set_begin(), max(mc.SET_LENGTHS), len(mc.SET_LENGTHS)
    points, inv = mc.normal_points(n, pi, n_point)
    K = 13 if n_point == 7 else 1
    st, ac, nx = soa(tr["state"]), soa(tr["action"]), soa(tr["stored"])
    runs = []
    for _ in range(2):
        obuf, out = guarded((n_set, K))
        sbuf, status = guarded((n_set,), torch.int32)
        sw.kernels.step_residual_normal_sets(p, dev(begin, torch.int64), longest, dev(points), st, ac, nx,
                                             inv_2e=dev(inv) if n_point == 7 else None,
                                             active=dev(np.array(mc.ACTIVE), torch.int32), out=out, status=status)
        torch.cuda.synchronize()
        assert intact(obuf) and intact(sbuf)
        runs.append((host(out), host(status)))
    (got, status), again = runs
    assert same(got, again[0]) and np.array_equal(status, again[1])
    for s in range(n_set):
        if not mc.ACTIVE[s]:
            assert (got[s] == mc.POISON).all() and status[s] == -77         # neither read nor written
            continue
        assert status[s] == 0
        q = sr.ratio(got[s], mc.normal_reference(n, pi, s, n_point))
        note(f"step_residual_normal_sets_kernel {n_point} point{'s' if n_point > 1 else ''}", n, q, f"set {s}")
        assert q <= 1.0, (s, q)
        if n_point == 7:
            JJ = got[s, 1:10].reshape(3, 3)
            assert same(JJ, JJ.T.copy())


def test_zz_every_instantiation_is_launched_and_the_figures_are_kept():
    """Last in the file.  The parametrisation above reaches all 115 entries of INSTANTIATIONS; when the whole file has
    run, the launches it made are those; and the observed figures are written out."""
    reached = mc.reached_by()
    assert all(callable(globals().get(name)) for name in reached)
    assert set().union(*map(set, reached.values())) == set(mc.INSTANTIATIONS) and len(mc.INSTANTIATIONS) == 115
    for test, over in (("test_step_accel_within_bounds", ("n", "model")),
                       ("test_env1_is_the_batched_kernel", ("n", "model")),
                       ("test_residual_single", ("n",)), ("test_residual_nt_forms", ("n",)),
                       ("test_residual_population", ("n",)), ("test_residual_sets", ("n",)),
                       ("test_residual_normal_sets", ("n", "n_point"))):
        marks = {m.args[0]: tuple(m.args[1]) for m in globals()[test].pytestmark if m.name == "parametrize"}
        want = {"n": mc.NS, "model": mc.MODELS, "n_point": mc.N_POINTS}
        assert marks == {k: want[k] for k in over}, test
    if os.environ.get(NT_OUT) or RAN != set(reached):
        return                                # the child, or a selection of the tests
    assert LAUNCHED == set(mc.INSTANTIATIONS), set(mc.INSTANTIATIONS) - LAUNCHED
    assert FIGURES and max(v["ratio"] for v in FIGURES.values()) <= 1.0
    r_oracle = {m: mc.r_oracle(m) for m in mc.MODELS}
    observed("step_matrix", {"R_oracle": r_oracle, "K": mc.K_MEASURED, "worst": dict(sorted(FIGURES.items()))})
