"""The RL-Glue ARS experiment (sw_rlglue_ars_run_f64, swimmer_amd.rlglue) without a GPU: the ABI, every argument
error, the wrapper's refusals, the parameter file, the delta stream, and the NumPy restatement (tests/rlglue_oracle.py)
against the reference's own runs (tests/golden/rlglue_ars.npz), exactly."""
import ctypes
import dataclasses
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rlglue_oracle  # noqa: E402
import swimmer_amd as sw  # noqa: E402
from swimmer_amd import rlglue  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")
TAGS = ("A", "B", "C", "D", "E", "F", "G", "SHIPPED", "CLIP1", "CLIP2")


def case_of(g, tag):
    seed, n, N, b, H, alpha, nu, max_u, h, it, l_i, k, m_i, dx, dy = g[f"{tag}_params"]
    return dict(seed=int(seed), n=int(n), N=int(N), b=int(b), H=int(H), alpha=alpha, nu=nu, max_u=max_u, h=h,
                iterations=int(it), l_i=l_i, k=k, m_i=m_i, direction=(dx, dy))


def test_entry_point_is_declared_and_exported():
    src = open(HEADER).read()
    assert ("int sw_rlglue_ars_run_f64(const sw_params *p, double max_u, int64_t n_agent, int64_t iter_begin, "
            "int32_t n_iter,") in src
    assert "sw_rlglue_ars_run_f64" in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), "sw_rlglue_ars_run_f64")
    assert sw._lib.load().sw_abi_version() == 3 and "#define SW_ABI_VERSION 3" in src
    assert sw._lib.load().sw_max_segments() == 8
    assert "swimmer_rlglue_ars.hip" in sw._build.SOURCES
    assert os.path.exists(os.path.join(sw._build.CSRC, "swimmer_rlglue_ars.hip"))
    assert sw.kernels.rlglue_ars_run is rlglue.kernels.rlglue_ars_run


def test_entry_point_validates_without_gpu():
    fn = sw._lib.load().sw_rlglue_ars_run_f64
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first

    def call(n=3, flags=sw._lib.FLAG_MODEL_TWIN, max_u=5.0, n_agent=5, iter_begin=0, n_iter=4, N=2, b=1, H=10,
             missing=None, no_params=False, **phys):
        p = sw.SwParams.make(n, flags=flags, **phys)
        # alpha nu deltas policy carry eval_returns train_returns status
        ptrs = [None if i == missing else dev for i in range(8)]
        return fn(None if no_params else ctypes.byref(p), max_u, n_agent, iter_begin, n_iter, N, b, H, *ptrs, None)
    assert call(no_params=True) == 1
    for missing in range(8):
        assert call(missing=missing) == 1
    assert call(missing=0, n_agent=0) == 1                               # NULL is reported first
    for bad in (dict(n_agent=0), dict(n_agent=-3), dict(n_agent=2 ** 31), dict(n_iter=-1), dict(iter_begin=-1),
                dict(N=0), dict(N=-2), dict(b=0), dict(b=3, N=2), dict(H=0), dict(H=-5)):
        assert call(**bad) == 3, bad
    assert call(flags=0) == 4                                            # the Gym model
    assert call(max_u=float("nan")) == 4 and call(max_u=-1e-9) == 4 and call(max_u=float("-inf")) == 4
    assert call(l_i=0.0) == 4 and call(m_i=float("inf")) == 4
    for n in (1, 9, 0, -1):
        assert call(n=n) == 2
    for n in range(2, 9):
        assert call(n=n, n_iter=0) == 0                                  # nothing to do, nothing written
    assert call(n_iter=0, max_u=float("inf"), b=2, N=2, iter_begin=7) == 0
    assert call(n_iter=0, max_u=0.0) == 0


W_A, W_IT, W_N, W_NSEG = 5, 3, 2, 4          # the wrapper tests' sizes: m = 3, d = 10


def _arguments():
    p = sw.SwParams.make(W_NSEG, flags=sw._lib.FLAG_MODEL_TWIN)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64)       # noqa: E731
    return p, dict(alpha=f(W_A), nu=f(W_A), deltas=f(W_IT, W_N, p.m, p.d, W_A), policy=f(p.m, p.d, W_A),
                   carry=f(p.m + 1, W_A), status=torch.zeros(W_A, dtype=torch.int32), eval_returns=f(W_IT, W_A),
                   train_returns=f(W_IT, 2 * W_N, W_A))


def _f64(*shape):
    return torch.zeros(shape, dtype=torch.float64)


# per parameter: wrong shape(s) -- the transposed and the off-by-one ones a caller would write --, wrong dtype,
# not contiguous, None where the tensor is required
BAD = {
    "alpha": [torch.zeros(W_A, dtype=torch.float32), _f64(2 * W_A)[::2]],
    "nu": [_f64(W_A + 1), _f64(W_A, 1), torch.zeros(W_A, dtype=torch.float32), _f64(2 * W_A)[::2], None],
    "deltas": [_f64(W_IT + 1, W_N, 3, 10, W_A), _f64(W_IT, W_N + 1, 3, 10, W_A), _f64(W_IT, W_N, 10, 3, W_A),
               _f64(W_IT, W_N, 3, 10, W_A - 1), _f64(W_IT, W_N, 3, 10), _f64(W_A, W_IT, W_N, 3, 10).permute(1, 2, 3, 4, 0),
               torch.zeros((W_IT, W_N, 3, 10, W_A), dtype=torch.float32), None],
    "policy": [_f64(10, 3, W_A), _f64(3, 10, W_A + 1), _f64(2, 10, W_A), _f64(W_A, 3, 10).permute(1, 2, 0),
               torch.zeros((3, 10, W_A), dtype=torch.float32), None],
    "carry": [_f64(3, W_A), _f64(5, W_A), _f64(W_A, 4), _f64(W_A, 4).t(), torch.zeros((4, W_A), dtype=torch.float32),
              None],
    "status": [torch.zeros(W_A, dtype=torch.int64), _f64(W_A), torch.zeros(W_A + 1, dtype=torch.int32),
               torch.zeros(2 * W_A, dtype=torch.int32)[::2], None],
    "eval_returns": [_f64(W_IT + 1, W_A), _f64(W_IT, W_A - 1), _f64(W_A, W_IT), _f64(W_A, W_IT).t(),
                     torch.zeros((W_IT, W_A), dtype=torch.float32)],
    "train_returns": [_f64(W_IT, W_N, W_A), _f64(W_IT, 2 * W_N + 1, W_A), _f64(W_IT, 2 * W_N, W_A + 1),
                      _f64(W_A, W_IT, 2 * W_N).permute(1, 2, 0), torch.zeros((W_IT, 2 * W_N, W_A), dtype=torch.float32)],
}


@pytest.fixture
def cpu_wrapper(monkeypatch):
    """The wrapper's checks on CPU tensors: the GPU requirement is taken out, and the foreign call is replaced by a
    recorder, so a call that passes every check is seen to reach it."""
    calls = []

    class Lib(object):
        @staticmethod
        def sw_rlglue_ars_run_f64(*args):
            calls.append(args)
            return 0
    monkeypatch.setattr(rlglue.kernels, "require_gpu", lambda: None)
    monkeypatch.setattr(rlglue.kernels, "_gpu", lambda t, name, ndim: (torch.device("cpu"), name))
    monkeypatch.setattr(rlglue.kernels, "load", lambda: Lib)
    monkeypatch.setattr(rlglue.kernels, "ptr", lambda t: t)
    monkeypatch.setattr(rlglue.kernels, "stream_ptr", lambda: None)
    return calls


@pytest.mark.parametrize("name,which", [(name, i) for name in sorted(BAD) for i in range(len(BAD[name]))])
def test_the_wrapper_names_the_bad_parameter(cpu_wrapper, name, which):
    p, kw = _arguments()
    kw[name] = BAD[name][which]
    with pytest.raises(sw.SwimmerHipError, match=rf"^{name}: expected a contiguous .* as alpha, got "):
        sw.kernels.rlglue_ars_run(p, 5.0, 0, W_IT, W_N, 1, 10, **kw)
    assert cpu_wrapper == []                                             # refused before the library


def test_the_wrapper_passes_good_tensors_and_allocates_the_outputs(cpu_wrapper):
    p, kw = _arguments()
    ev, tr = sw.kernels.rlglue_ars_run(p, 5.0, 2, W_IT, W_N, 1, 10, **kw)
    assert ev is kw["eval_returns"] and tr is kw["train_returns"] and len(cpu_wrapper) == 1
    args = cpu_wrapper[0]
    assert args[1:8] == (5.0, W_A, 2, W_IT, W_N, 1, 10)                  # max_u n_agent iter_begin n_iter N b H
    assert [a is t for a, t in zip(args[8:16], (kw["alpha"], kw["nu"], kw["deltas"], kw["policy"], kw["carry"], ev, tr,
                                                kw["status"]))] == [True] * 8
    del kw["eval_returns"], kw["train_returns"]
    ev, tr = sw.kernels.rlglue_ars_run(p, 5.0, 0, W_IT, W_N, 1, 10, **kw)
    assert ev.shape == (W_IT, W_A) and tr.shape == (W_IT, 2 * W_N, W_A)
    assert ev.dtype == tr.dtype == torch.float64 and ev.is_contiguous() and tr.is_contiguous()
    assert cpu_wrapper[1][13] is ev and cpu_wrapper[1][14] is tr


def test_without_a_gpu_tensor_the_wrapper_refuses_at_once(monkeypatch):
    monkeypatch.setattr(rlglue.kernels, "require_gpu", lambda: None)
    p, kw = _arguments()
    with pytest.raises(sw.SwimmerHipError, match="^alpha: expected a 1-D tensor on the GPU"):   # host tensors
        sw.kernels.rlglue_ars_run(p, 5.0, 0, W_IT, W_N, 1, 10, **kw)
    kw["alpha"] = None
    with pytest.raises(sw.SwimmerHipError, match="^alpha: expected a 1-D tensor on the GPU"):
        sw.kernels.rlglue_ars_run(p, 5.0, 0, W_IT, W_N, 1, 10, **kw)


def test_experiment_refuses_bad_parameters():
    for bad in (dict(n_seg=1), dict(n_seg=9), dict(N=0), dict(b=0), dict(b=2, N=1), dict(H=0), dict(max_u=-1.0),
                dict(max_u=float("nan"))):
        with pytest.raises(ValueError):
            rlglue.SwimmerExperimentBatch(rlglue.Parameters(**bad), [0])
    with pytest.raises(ValueError):
        rlglue.SwimmerExperimentBatch(rlglue.Parameters(), [])
    with pytest.raises(ValueError):
        rlglue.SwimmerExperimentBatch(rlglue.Parameters(), [0, 1], alphas=[0.1])


def test_parameters_round_trip(tmp_path):
    path = tmp_path / "parameters.txt"
    # the reference's format: key value..., any order, keys nobody knows, "5." and "0." as it writes them
    path.write_text("H 250\nn_seg 5\ndirection 0. -1.0\ncomment this is ignored\nh_global 0.005\nN 4\n\nb 2\n"
                    "alpha 0.03\nnu 0.04\nmax_u 5.\nl_i 1.\nk 10.\nm_i 1.5\n")
    p = rlglue.Parameters.load(path)
    assert p == rlglue.Parameters(n_seg=5, direction=(0.0, -1.0), h_global=0.005, N=4, b=2, H=250, alpha=0.03,
                                  nu=0.04, max_u=5.0, l_i=1.0, k=10.0, m_i=1.5)
    assert [f.name for f in dataclasses.fields(p)] == ["n_seg", "direction", "h_global", "N", "b", "H", "alpha", "nu",
                                                      "max_u", "l_i", "k", "m_i"]
    out = tmp_path / "saved.txt"
    p.save(out)
    assert rlglue.Parameters.load(out) == p
    odd = rlglue.Parameters(alpha=1e-5 / 3, nu=2.0 ** -40, max_u=float("inf"), h_global=0.1 + 0.2)
    odd.save(out)
    assert rlglue.Parameters.load(out) == odd
    for line in out.read_text().splitlines():                             # what the reference's readers take
        tokens = line.split(" ")
        assert len(tokens) == (3 if tokens[0] == "direction" else 2)
        (int if tokens[0] in ("n_seg", "N", "b", "H") else float)(tokens[1])
    part = tmp_path / "part.txt"
    part.write_text("N 3\n")
    assert rlglue.Parameters.load(part) == rlglue.Parameters(N=3)         # the rest: the shipped file's values
    assert rlglue.Parameters() == rlglue.Parameters(3, (1.0, 0.0), 0.01, 1, 1, 1000, 0.02, 0.02, 5.0, 1.0, 10.0, 1.0)


def test_delta_stream_order_and_position(golden, monkeypatch):
    """The batch draws what the agent draws: N matrices at start, N after every iteration, from a generator per seed
    (never NumPy's global one); after run(k) its stream stands where the reference's stood."""
    g = golden.rlglue_ars
    monkeypatch.setattr(sw._lib, "require_gpu", lambda: None)
    seen = []                                   # the launch is replaced: host tensors in, zeros out

    def fake_run(p, max_u, iter_begin, n_iter, N, b, H, alpha, nu, deltas, policy, carry, status):
        seen.append((iter_begin, deltas.numpy().copy()))
        return torch.zeros((n_iter, alpha.shape[0])), torch.zeros((n_iter, 2 * N, alpha.shape[0]))
    monkeypatch.setattr(rlglue.kernels, "rlglue_ars_run", fake_run)
    np.random.seed(12345)
    before = np.random.get_state()[1].copy()
    for tag in ("B", "C"):
        c = case_of(g, tag)
        seen.clear()
        params = rlglue.Parameters(n_seg=c["n"], N=c["N"], b=c["b"], H=c["H"])
        ex = rlglue.SwimmerExperimentBatch(params, [c["seed"], c["seed"] + 1], device="cpu")
        ex.run(2)
        ex.run(c["iterations"] - 2)
        fed = np.concatenate([d for _, d in seen], axis=0)               # [iterations, N, m, d, 2]
        assert [b for b, _ in seen] == [0, 2]
        assert np.array_equal(fed[..., 0], g[f"{tag}_deltas"][:-1])
        assert np.array_equal(ex._pending[..., 0], g[f"{tag}_deltas"][-1])
        assert ex._rng[0].rand() == g[f"{tag}_next_rand"]
        other = np.random.RandomState(c["seed"] + 1).rand(c["iterations"] + 1, c["N"], c["n"] - 1, 2 * c["n"] + 2)
        assert np.array_equal(fed[..., 1], other[:-1])
    assert np.array_equal(np.random.get_state()[1], before)              # the global generator is untouched


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference(golden, tag):
    g = golden.rlglue_ars
    c = case_of(g, tag)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # G: the reference's own 0 / 0
        run = rlglue_oracle.Run(c["n"], c["N"], c["b"], c["H"], c["alpha"], c["nu"], c["max_u"], g[f"{tag}_deltas"],
                                c["l_i"], c["m_i"], c["k"], c["h"], c["direction"]).run(c["iterations"])
    got = run.arrays()
    assert np.array_equal(got["eval"], g[f"{tag}_eval"])
    assert np.array_equal(got["rew"], g[f"{tag}_rew"])
    assert np.array_equal(got["policies"], g[f"{tag}_policies"], equal_nan=True)
    assert np.array_equal(got["clips"], g[f"{tag}_clips"])


def test_golden_covers_what_it_must(golden):
    g = golden.rlglue_ars
    cases = {tag: case_of(g, tag) for tag in TAGS}
    assert {c["n"] for c in cases.values()} == {2, 3, 4, 5, 6, 8}
    assert {c["N"] for c in cases.values()} == {1, 2, 3}
    assert {(c["b"], c["N"] >= 2) for c in cases.values()} >= {(1, False), (1, True), (2, True)}
    hs = {c["H"] for c in cases.values()}
    assert {1, 2, 1000} <= hs and any(10 <= h <= 40 for h in hs)
    s = cases["SHIPPED"]
    assert (s["n"], s["N"], s["b"], s["H"], s["alpha"], s["nu"], s["max_u"], s["h"], s["iterations"]) == \
        (3, 1, 1, 1000, 0.02, 0.02, 5.0, 0.01, 3)
    for tag, c in cases.items():
        assert c["iterations"] == 3 if tag == "SHIPPED" else c["iterations"] == 1 if tag == "G" else \
            4 <= c["iterations"] <= 6
        if tag != "G":
            assert 0 < g[f"{tag}_sens_policies"] <= 1e-7 and g[f"{tag}_sens_eval"] > 0
        assert g[f"{tag}_sens_rew"] > 0
    for tag in ("CLIP1", "CLIP2"):
        clips = g[f"{tag}_clips"]
        assert clips.min() >= 0.1 * clips.sum()
    for tag in ("A", "B", "C", "D", "E", "F", "SHIPPED"):
        assert g[f"{tag}_clips"][:2].sum() == 0
