"""CACLA without a GPU: the NumPy restatement (tests/cacla_oracle.py) against the reference's own runs
(tests/golden/cacla.npz), the host side's random streams, the C entry point's declaration and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import swimmer_amd as sw
from conftest import GOLDEN, ROOT
from swimmer_amd import cacla

import cacla_oracle

HEADER = os.path.join(ROOT, "include", "swimmer_hip.h")
CASES = ("A", "B", "C", "D", "E", "A0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cacla.npz"), allow_pickle=False)


def case_of(gold, tag):
    seed, n, gamma, alpha, sigma, steps, train = gold[f"{tag}_hyper"]
    return dict(seed=int(seed), n=int(n), gamma=gamma, alpha=alpha, sigma=sigma, steps=int(steps), train=bool(train),
                **{k: gold[f"{tag}_{k}"] for k in ("w0", "w1", "noise", "rewards", "state", "next_normal", "next_rand")})


@pytest.mark.parametrize("tag", CASES)
def test_oracle_reproduces_the_reference(gold, tag):
    """Every case, every step; 1e-12 absolute on rewards, final weights and the swimmer's state."""
    c = case_of(gold, tag)
    got = cacla_oracle.run(c["n"], c["gamma"], c["alpha"], c["w0"], c["noise"], train=c["train"])
    err_r = np.abs(got["rewards"] - c["rewards"]).max()
    err_w = np.abs(got["weights"] - c["w1"]).max()
    err_s = np.abs(got["state"] - c["state"]).max()
    print(f"case {tag}: rewards {err_r:.3g} weights {err_w:.3g} state {err_s:.3g}")
    assert got["rewards"].shape == (c["steps"],)
    assert err_r <= 1e-12 and err_w <= 1e-12 and err_s <= 1e-12
    if not c["train"]:
        assert np.array_equal(got["weights"], c["w0"])


@pytest.mark.parametrize("tag", CASES)
def test_host_streams_are_the_references(gold, tag):
    """The initial weights from torch's global generator and from a torch.Generator, the noise from NumPy's global
    stream and from a RandomState, drawn in chunks of odd size: all equal to what the reference's run drew, and the
    streams are left where the reference leaves them."""
    c = case_of(gold, tag)
    n, m, T = c["n"], c["n"] - 1, c["steps"]
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    assert np.array_equal(cacla.draw_networks(n), c["w0"])
    cov = c["sigma"] * np.identity(m)
    noise = np.concatenate([np.random.multivariate_normal(np.zeros(m), cov, size=k) for k in (37, T - 37)])
    assert np.array_equal(noise, c["noise"])
    assert np.random.standard_normal() == c["next_normal"]
    assert np.array_equal(torch.rand(1).numpy(), c["next_rand"])
    # the batch's private generators give the same, and leave the global ones alone
    before = torch.get_rng_state(), np.random.get_state()[1].copy()
    assert np.array_equal(cacla.draw_networks(n, torch.Generator().manual_seed(c["seed"])), c["w0"])
    rs = np.random.RandomState(c["seed"])
    assert np.array_equal(rs.multivariate_normal(np.zeros(m), cov, size=T), c["noise"])
    assert torch.equal(torch.get_rng_state(), before[0]) and np.array_equal(np.random.get_state()[1], before[1])


def test_entry_point_is_declared_and_exported():
    src = open(HEADER).read()
    assert "int sw_cacla_run_f64(const sw_params *p, int64_t n_agent, int32_t n_iter, int32_t train," in src
    assert "#define SW_CACLA_HIDDEN 12" in src
    assert "sw_cacla_run_f64" in sw._lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(sw._lib.library_path()), "sw_cacla_run_f64")
    assert sw._lib.load().sw_abi_version() == 3
    assert "swimmer_cacla.hip" in sw._build.SOURCES


def test_entry_point_validates_without_gpu():
    fn = sw._lib.load().sw_cacla_run_f64
    ok = sw.SwParams.make(3)
    dev = ctypes.c_void_p(8)          # never dereferenced: validation comes first

    def call(p, n_agent=5, n_iter=16, missing=None):
        ptrs = [None if i == missing else dev for i in range(6)]       # gamma alpha noise weights state rewards
        return fn(ctypes.byref(p) if p is not None else None, n_agent, n_iter, 1, *ptrs, None, None, None)
    assert call(None) == 1
    for missing in range(6):
        assert call(ok, missing=missing) == 1
    assert call(ok, n_agent=0) == 3
    assert call(ok, n_agent=-4) == 3
    assert call(ok, n_agent=2 ** 31) == 3
    assert call(ok, n_iter=-1) == 3
    assert call(sw.SwParams.make(3, flags=4)) == 4                      # twin model
    assert call(sw.SwParams.make(9)) == 2
    assert call(sw.SwParams.make(1)) == 2
    assert call(ok, n_iter=0) == 0                                      # nothing to do, nothing written


def test_net_doubles_agrees_with_the_header():
    src = open(HEADER).read()
    hidden = int(re.search(r"#define SW_CACLA_HIDDEN (\d+)", src).group(1))
    body = re.search(r"#define SW_CACLA_NET_DOUBLES\(n\) (.*)", src).group(1)
    for n in range(2, 9):
        want = eval(body, {"SW_CACLA_HIDDEN": hidden, "n": n})          # the macro is plain integer arithmetic
        d = 2 * n + 2
        assert want == cacla.net_doubles(n) == sw.kernels.cacla_net_doubles(n) == cacla_oracle.net_doubles(n)
        vec = np.arange(want, dtype=np.float64)
        w1, b1, w2, b2 = cacla.unpack_net(vec, d)
        assert w1.shape == (hidden, d) and w1[1, 0] == d and b1[0] == hidden * d and w2[0] == hidden * d + hidden
        assert b2 == want - 1
        assert np.array_equal(cacla.pack_net(w1, b1, w2, b2), vec)
