"""The reference's native twin (rlglue/environment/SwimmerEnvironment.cpp): oracle pinned by
the two reference-authored known answers, HIP model (SW_FLAG_MODEL_TWIN) against the oracle,
and the RL-Glue plug-in ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from conftest import ROOT

# rlglue/test/acceleration-compare.txt:5 / swimmer-compare.txt:22 (state), torque = max_u/2
KAT_STATE = [-0.0453422, 1.33766e-11, -1.35003, -1.4868, 1.5708, -1.88179e-15, -1.79156, 1.4868]
KAT_TORQUE = [2.5, 2.5]
KAT_GDD = [-2.05622, -0.0173465]                      # acceleration-compare.txt:102
KAT_TDD = [3.97741, 14.2667, 19.7878]                 # acceleration-compare.txt:103
KAT_NEXT = [-0.0515109, -5.20396e-05, -1.35445, -1.47487, 1.57093, 0.0428002, -1.78692, 1.54616]
KAT_H = 0.003                                          # swimmer-compare.txt:100 (recorded run)
PKG = os.path.join(ROOT, "safe-exploration-with-simulator-in-rl-algorithms_amd")


def sig6(x, ref):
    """agreement to the 6 significant digits the reference printed"""
    return np.all(np.abs(np.asarray(x) - np.asarray(ref)) <= 5.1e-6 * np.maximum(np.abs(ref), 1e-30) + 1e-16)


def test_oracle_reproduces_reference_recorded_outputs():
    p = oracle.OracleParams.make(3, 1.0, 1.0, 10.0, KAT_H)
    g, t = oracle.twin_accelerations(p, KAT_STATE, KAT_TORQUE)
    assert sig6(g, KAT_GDD) and sig6(t, KAT_TDD)
    nxt, r = oracle.twin_step(p, KAT_STATE, KAT_TORQUE)
    assert sig6(nxt, KAT_NEXT)
    assert r == nxt[0]                                 # direction (1, 0)
    # not Coulom's / the Gym env's model: same state, different accelerations
    g_gym, _ = oracle.accelerations(p, KAT_STATE, KAT_TORQUE)
    assert abs(g_gym[0] - g[0]) > 1.0


def test_oracle_assembly_vs_the_recorded_matrix_entry_by_entry():
    """rlglue/test/acceleration-compare.txt:27-43 (A), :46-62 (B), :84-100 (X): the reference's
    own printout of the 17 x 17 system for the known-answer state (tests/golden/twin_kat.json,
    extracted by tests/golden/make_twin_kat.py).  Every entry of the restatement's assembled
    A and B and every component of its solution agree to the 6 digits printed -- so the
    formulation the n != 3 comparisons rest on is pinned entry by entry at n = 3, not just
    through two derived numbers."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "twin_kat.json")) as f:
        rec = json.load(f)
    assert rec["state"] == KAT_STATE and rec["torque"] == KAT_TORQUE
    p = oracle.OracleParams.make(rec["n"], rec["l_i"], rec["m_i"], rec["k"], KAT_H)
    A, B, X = oracle.twin_system(p, rec["state"], rec["torque"])
    Ar, Br, Xr = np.array(rec["A"]), np.array(rec["B"]), np.array(rec["X"])
    assert A.shape == (17, 17)
    # structure: exactly the recorded sparsity pattern (zeros are printed as 0)
    assert np.array_equal(A != 0.0, Ar != 0.0)
    assert np.abs(A - Ar).max() <= 5.1e-6 * np.abs(Ar).max()
    assert sig6(A[Ar != 0.0], Ar[Ar != 0.0])
    # B: rounding-level entries are printed as 1.8e-15 / 0; compare absolutely at 6 digits of the scale
    assert np.abs(B - Br).max() <= 5.1e-6 * np.abs(Br).max()
    assert sig6(B[np.abs(Br) > 1e-3], Br[np.abs(Br) > 1e-3])
    assert np.abs(X - Xr).max() <= 5.1e-6 * np.abs(Xr).max()
    assert sig6(X[np.abs(Xr) > 1e-3], Xr[np.abs(Xr) > 1e-3])
    assert sig6(X[:3], rec["angle_accelerations"])
    # G_dotdot is the mean of the three Gdd_i the solution holds (SwimmerEnvironment.cpp:222-225)
    assert sig6([X[11::2].mean(), X[12::2].mean()], rec["G_dotdot"])


def test_rlglue_plugin_exports_the_five_entry_points():
    lib = ctypes.CDLL(os.path.join(PKG, "csrc", "librlglue_swimmer_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "rlglue_swimmer.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(env_[a-z]+)\s*\(", hdr)))
    assert names == ["env_cleanup", "env_init", "env_message", "env_start", "env_step"]
    for n in names:
        assert hasattr(lib, n)


def random_states(rng, n, B):
    st = np.empty((B, 2 * n + 2))
    st[:, 0:2] = rng.uniform(-0.5, 0.5, (B, 2))
    st[:, 2::2] = rng.uniform(-np.pi, np.pi, (B, n))
    st[:, 3::2] = rng.uniform(-2, 2, (B, n))
    return st, rng.uniform(-5, 5, (B, n - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_hip_twin_model_vs_oracle(n):
    import torch
    import swimmer_amd as sw
    rng = np.random.default_rng(n)
    for l, m, k, h, d in ((1.0, 1.0, 10.0, 0.01, (1.0, 0.0)), (0.8, 1.2, 10.2, 0.003, (0.6, -0.8))):
        st, ac = random_states(rng, n, 257)
        op = oracle.OracleParams.make(n, l, m, k, h, d)
        ref, ref_r = oracle.twin_step_batch(op, st, ac)
        p = sw.SwParams.make(n, l, m, k, h, d, flags=sw._lib.FLAG_MODEL_TWIN)
        dev = "cuda:0"
        sd = torch.as_tensor(np.ascontiguousarray(st.T), device=dev)
        ad = torch.as_tensor(np.ascontiguousarray(ac.T), device=dev)
        status = torch.zeros(st.shape[0], dtype=torch.int32, device=dev)
        nxt, rew = sw.kernels.step(p, sd, ad, status=status)
        gdd, tdd = sw.kernels.accelerations(p, sd, ad)
        assert int(status.abs().sum()) == 0
        assert np.abs(nxt.T.cpu().numpy() - ref).max() <= 1e-11
        assert np.abs(rew.cpu().numpy() - ref_r).max() <= 1e-11
        for b in (0, 100, 256):
            g, t = oracle.twin_accelerations(op, st[b], ac[b])
            assert np.abs(gdd[:, b].cpu().numpy() - g).max() <= 1e-11 * max(1.0, np.abs(g).max())
            assert np.abs(tdd[:, b].cpu().numpy() - t).max() <= 1e-11 * max(1.0, np.abs(t).max())


@pytest.mark.gpu
def test_hip_twin_known_answers_and_rollout():
    import torch
    import swimmer_amd as sw
    dev = "cuda:0"
    p = sw.SwParams.make(3, 1.0, 1.0, 10.0, KAT_H, flags=sw._lib.FLAG_MODEL_TWIN)
    sd = torch.as_tensor(np.array(KAT_STATE).reshape(-1, 1), device=dev)
    ad = torch.as_tensor(np.array(KAT_TORQUE).reshape(-1, 1), device=dev)
    gdd, tdd = sw.kernels.accelerations(p, sd, ad)
    nxt, _ = sw.kernels.step(p, sd, ad)
    assert sig6(gdd[:, 0].cpu().numpy(), KAT_GDD) and sig6(tdd[:, 0].cpu().numpy(), KAT_TDD)
    assert sig6(nxt[:, 0].cpu().numpy(), KAT_NEXT)
    # reset state of the twin = env_start's all-0.001 (SwimmerEnvironment.cpp:39-42)
    assert torch.equal(sw.kernels.reset(p, 3), torch.full((8, 3), 0.001, dtype=torch.float64, device=dev))
    # rollouts (lane kernel, linear policy, start = 0.001) vs stepping the oracle
    rng = np.random.default_rng(0)
    R, H = 70, 200
    pol = 0.5 * rng.uniform(-1, 1, (R, 2, 8))
    p2 = sw.SwParams.make(3, 1.0, 1.0, 10.0, 0.01, flags=sw._lib.FLAG_MODEL_TWIN)
    traj = torch.empty((H, 8, R), dtype=torch.float64, device=dev)
    ret = sw.kernels.rollout(p2, H, torch.as_tensor(pol, device=dev), traj=traj)
    op = oracle.OracleParams.make(3, 1.0, 1.0, 10.0, 0.01)
    for r in (0, 33, 69):
        s, tot = np.full(8, 0.001), 0.0
        for t in range(H):
            s, rew = oracle.twin_step(op, s, pol[r] @ s)
            tot += rew
            assert np.abs(traj[t, :, r].cpu().numpy() - s).max() <= 1e-9
        assert abs(float(ret[r]) - tot) <= 1e-9


class _Abs(ctypes.Structure):
    _fields_ = [("numInts", ctypes.c_uint), ("numDoubles", ctypes.c_uint), ("numChars", ctypes.c_uint),
                ("intArray", ctypes.POINTER(ctypes.c_int)), ("doubleArray", ctypes.POINTER(ctypes.c_double)),
                ("charArray", ctypes.c_char_p)]


class _ROT(ctypes.Structure):
    _fields_ = [("reward", ctypes.c_double), ("observation", ctypes.POINTER(_Abs)), ("terminal", ctypes.c_int)]


@pytest.mark.gpu
def test_rlglue_plugin_end_to_end(tmp_path, monkeypatch):
    import torch  # noqa: F401  (loads the HIP runtime the plug-in shares)
    lib = ctypes.CDLL(os.path.join(PKG, "csrc", "librlglue_swimmer_hip.so"))
    lib.env_init.restype = ctypes.c_char_p
    lib.env_message.restype = ctypes.c_char_p
    lib.env_message.argtypes = [ctypes.c_char_p]
    lib.env_start.restype = ctypes.POINTER(_Abs)
    lib.env_step.restype = ctypes.POINTER(_ROT)
    lib.env_step.argtypes = [ctypes.POINTER(_Abs)]
    # parameter file in the reference's format (rlglue/parameters.txt)
    pf = tmp_path / "parameters.txt"
    pf.write_text("n_seg 3\ndirection 1.0 0.\nh_global 0.01\nN 1\nb 1\nH 1000\nalpha 0.02\nnu 0.02\n"
                  "max_u 5.\nl_i 1.\nk 10.\nm_i 1.\n")
    monkeypatch.setenv("SWIMMER_PARAMETERS", str(pf))
    msg = lib.env_message(b"set parameters").decode()
    assert msg == ("Environment parameters are: n_seg=3; max_u=5.000000; l_i=1.000000; k=10.000000; "
                   "m_i=1.000000; h_global=0.010000")
    spec = lib.env_init().decode()
    assert spec == ("VERSION RL-Glue-3.0 PROBLEMTYPE continuing DISCOUNTFACTOR 0.9 OBSERVATIONS DOUBLES "
                    "(8 UNSPEC UNSPEC) ACTIONS DOUBLES (2 -5.000000 5.000000) REWARDS (UNSPEC UNSPEC) "
                    "EXTRA SwimmerEnvironment(C++) by Leon Zheng")
    assert lib.env_message(b"what is your name?") == b"My name is swimmer_environment, C++ edition!"
    obs = lib.env_start().contents
    assert obs.numDoubles == 8 and [obs.doubleArray[i] for i in range(8)] == [0.001] * 8
    op = oracle.OracleParams.make(3, 1.0, 1.0, 10.0, 0.01)
    s = np.full(8, 0.001)
    torque = (ctypes.c_double * 2)()
    act = _Abs(0, 2, 0, None, torque, None)
    rng = np.random.default_rng(1)
    for t in range(25):
        u = rng.uniform(-5, 5, 2)
        torque[0], torque[1] = u
        ro = lib.env_step(ctypes.byref(act)).contents
        s, r = oracle.twin_step(op, s, u)
        got = np.array([ro.observation.contents.doubleArray[i] for i in range(8)])
        assert np.abs(got - s).max() <= 1e-10 and abs(ro.reward - r) <= 1e-10 and ro.terminal == 0
        if t == 9:
            assert lib.env_message(b"save state").startswith(b"saved_observation")
            saved = s.copy()
    assert lib.env_message(b"load state").startswith(b"this_observation")
    s = saved
    torque[0], torque[1] = 1.0, -2.0
    ro = lib.env_step(ctypes.byref(act)).contents
    s, r = oracle.twin_step(op, s, [1.0, -2.0])
    got = np.array([ro.observation.contents.doubleArray[i] for i in range(8)])
    assert np.abs(got - s).max() <= 1e-10
    assert lib.env_message(b"hello?") == b"SwimmerEnvironment(C++) does not respond to that message."
    lib.env_cleanup()
