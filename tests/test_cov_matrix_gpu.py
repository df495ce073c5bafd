"""The covariance family on the GPU against the long-double reference of tests/cov_matrix_cases.py, inside the
derived per-entry bound ((1 + u)^L - 1 + 2^-59) A of that file (the 2^-59 is the reference's own rounding;
tests/test_cov_matrix_cpu.py checks that the cases reach the paths and that the bound would show the mistakes it is
there for).

STANDALONE PASS (sw_traj_moments_f64, traj_moments_kernel<2 n + 2, 256>, n = 2..8).  Every tile length from 1 to 13
steps, one rollout up to one past a full column tile, the merge at n_tiles 1 .. 330 and 4097, three data regimes.
acc is a view of exactly sw_cov_acc_doubles doubles between guard entries, traj a view between NaN; a second run into a
fresh accumulator has the same bits; a pass into a pre-filled acc is fl(acc0 + fresh) bit for bit; two passes of
different shapes share one acc; the ticket is zero again behind every pass; regime c is bit-exact.

OWED PASSES (tiling with riding = true).  A rollout launch of the ARS pipeline leaves the pass over its trajectories
owed; the next launch of the same form carries it as extra workgroups (side_cov_tile<D, BLOCK>), or
sw_ars_pipeline_sync_cov flushes it (traj_moments_kernel<D, BLOCK> with the owed block: 128 threads behind the
mirror-quad form, 64 behind the quad form, 256 behind the row and lane forms).  To make such a pass sum data of the
test's choosing:
    launch k     rollouts with traj_A and cov_acc: the pass over traj_A is owed
    copy         traj_A <- the regime's data, on the same stream
    launch k+1   rollouts with traj_B (the pass rides here) -- or sync_cov() (the pass is flushed)
The three are enqueued on one stream, which runs them in order: the copy starts when launch k has stored its last
trajectory entry and is complete before a workgroup of launch k + 1, or of the flush, exists.  So the pass reads the
copied data and nothing else, and cov_acc is the reference of that data.  The ride and the flush must agree bit for bit,
and launch k + 1's own outputs must be those of the same rollouts through sw_ars_rollouts_f64, which carries no side job.

The quad form takes batches of up to 8192 rollouts only with SWIMMER_N3_KERNEL=quad, which the library reads once per
process: its cases run in a child process (as in tests/test_rollout_matrix_gpu.py), and once more here at 8194 rollouts,
where the dispatch picks it by itself.

The worst |got - ref| / (u A) per kernel form goes to conftest.observed (profiles/cov_matrix_observed.json): a record,
not a limit.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import observed

import cov_matrix_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 517                     # doubles in front of and behind acc and traj
SENTINEL = -1234567.0
QUAD_ENV = os.environ.get("SWIMMER_N3_KERNEL", "")[:1] == "q"       # this process runs n = 3 on the quad kernel
OBSERVED = "cov_matrix_quad" if QUAD_ENV else "cov_matrix"
_seen = {}


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert not mc.knobs_set(), "%s is set: it changes the tiling under test" % mc.knobs_set()
    return swimmer_amd


def _note(key, r):
    _seen[key] = max(_seen.get(key, 0.0), float(r))


def _keep():
    observed(OBSERVED, dict(sorted(_seen.items())))


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=DEV)


class Acc(object):
    """An accumulator of exactly `size` doubles between two margins of SENTINEL; zero, or acc0 in its sums."""

    def __init__(self, size, acc0=None):
        self.size = size
        self.whole = torch.full((size + 2 * MARGIN,), SENTINEL, dtype=torch.float64, device=DEV)
        self.t = self.whole[MARGIN:MARGIN + size]
        self.t.zero_()
        if acc0 is not None:
            self.t[:len(acc0)].copy_(_dev(acc0))

    def sums(self, D):
        """count | S1 | S2 on the host, after the guards and the ticket have been looked at."""
        torch.cuda.synchronize()
        assert bool((self.whole[:MARGIN] == SENTINEL).all()) and bool((self.whole[MARGIN + self.size:] == SENTINEL).all())
        assert int(self.t[mc.cov_sums(D):mc.cov_sums(D) + 1].view(torch.int64)[0]) == 0, "the ticket is not back at 0"
        return self.t[:mc.cov_sums(D)].cpu().numpy().copy()

    def check_tiles(self, D, host, t, what):
        """Regime c: the scratch rows a pass leaves behind hold every tile's own sums, transposed (entry j of tile i at
        [j n_tiles + i]).  The S2[0, 0] entries must be the tiles' exact partial sums in tile order, and nothing lies
        behind the last row: the pass took the tiling t -- its block's columns, its tchunk, tile = by nbx + bx."""
        rows = self.t[mc.cov_sums(D) + 1:].cpu().numpy()
        W = D + D * D
        assert np.array_equal(rows[D * t.n_tiles:(D + 1) * t.n_tiles], mc.tile_partials(host, t)), (what, "tiles")
        assert not rows[W * t.n_tiles:].any(), (what, "scratch behind the last row")


class Traj(object):
    """A trajectory buffer [H, D, R] between two margins of NaN."""

    def __init__(self, shape, data=None):
        numel = int(np.prod(shape))
        self.whole = torch.full((numel + 2 * MARGIN,), float("nan"), dtype=torch.float64, device=DEV)
        self.t = self.whole[MARGIN:MARGIN + numel].view(shape)
        if data is not None:
            self.t.copy_(data if isinstance(data, torch.Tensor) else _dev(data))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check(key, what, got, ref, L, exact):
    """The ratio is kept before anything is asserted."""
    _note(key, max(mc.ratios(got, ref)))
    bad = mc.violations(got, ref, L)
    if bad:
        _keep()
    assert not bad, (what, L, bad)
    if exact:
        assert np.array_equal(got, mc.packed(ref)), (what, "regime c is exact")


def _prefill(D):
    """Known sums of an earlier life of the accumulator, not symmetric on purpose."""
    k = np.arange(mc.cov_sums(D), dtype=np.float64)
    return 3.0 + 0.37 * k - 0.011 * k * k


def _standalone(sw, p, D, traj, size, acc0=None, acc=None):
    acc = acc or Acc(size, acc0)
    sw.kernels.traj_moments(p, traj.t, acc.t)
    return acc.sums(D)


def _standalone_case(sw, n, R, H, regimes=mc.REGIMES):
    """One shape of the standalone pass in every regime: bound, exactness, same bits again, pre-filled acc."""
    p = sw.SwParams.make(n)
    D = mc.dims(n)
    t = mc.tiling(R, H, mc.MOM_BLOCK, D, False)
    L = mc.additions(t, mc.MOM_BLOCK, D)
    size = sw.kernels.cov_acc_doubles(p, R, H)
    assert size == mc.acc_doubles(n, R, H) >= mc.cov_sums(D) + 1 + t.n_tiles * (D + D * D)
    key = "standalone/traj_moments_kernel_" + mc.form_name(D, mc.MOM_BLOCK)
    for regime in regimes:
        host = mc.data(regime, n, H, R)
        ref = mc.reference_for(regime, host)
        traj = Traj(host.shape, host)
        what = (n, R, H, regime, t.n_tiles)
        first = _standalone(sw, p, D, traj, size)
        _check(key, what, first, ref, L, regime == "c")
        if regime == "c":
            acc = Acc(size)
            _standalone(sw, p, D, traj, size, acc=acc)
            acc.check_tiles(D, host, t, what)
        again = _standalone(sw, p, D, traj, size)
        assert np.array_equal(_bits(first), _bits(again)), what
        acc0 = _prefill(D)
        pre = _standalone(sw, p, D, traj, size, acc0)
        assert np.array_equal(_bits(pre), _bits(acc0 + first)), (what, "pre-filled")
    return key


@pytest.mark.parametrize("n", mc.NS, ids=lambda n: "traj_moments_kernel_" + mc.form_name(mc.dims(n), mc.MOM_BLOCK))
def test_standalone_pass_at_every_short_tile(sw, n):
    """H = 1..11 and 13 (tiles of 1..8 steps, the split form's prologue and every tail as the whole tile), R around
    one column tile, three regimes."""
    for R, H in mc.standalone_shapes(n):
        _standalone_case(sw, n, R, H)
    _keep()


@pytest.mark.parametrize("n,R,H", mc.MERGE_CASES, ids=[
    "traj_moments_kernel_%s-R%d-H%d-%dtiles" % (mc.form_name(mc.dims(n), mc.MOM_BLOCK), R, H,
                                                mc.tiling(R, H, mc.MOM_BLOCK, mc.dims(n), False).n_tiles)
    for n, R, H in mc.MERGE_CASES])
def test_standalone_merge_at_every_tile_count(sw, n, R, H):
    """traj_moments_kernel<8, 256> (n = 3, wide) and <14, 256> (n = 6, split): the last tile's merge with its four
    interleaved partials, three-step tail and clamped last group of entries, at n_tiles 1 .. 322."""
    _standalone_case(sw, n, R, H)
    _keep()


@pytest.mark.parametrize("regime", mc.REGIMES)
def test_standalone_pass_beyond_the_tile_cap(sw, regime):
    """n = 5, 262145 rollouts x 2 steps: 4097 column tiles, more than the cap, which then leaves ny = 1."""
    n, R, H = mc.CAP_CASE
    assert mc.tiling(R, H, mc.MOM_BLOCK, mc.dims(n), False).n_tiles == 4097
    _standalone_case(sw, n, R, H, regimes=(regime,))
    _keep()


@pytest.mark.parametrize("n,first,second", mc.TWO_SHAPE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_two_passes_of_different_shapes_share_one_acc(sw, n, first, second):
    """The ticket is back at zero and the scratch rows are laid out anew by n_tiles: the second pass adds its own
    reference, bit for bit what it gives into a fresh accumulator."""
    p = sw.SwParams.make(n)
    D = mc.dims(n)
    size = max(sw.kernels.cov_acc_doubles(p, *s) for s in (first, second))
    key = "standalone/traj_moments_kernel_" + mc.form_name(D, mc.MOM_BLOCK)
    for regime in ("a", "c"):
        acc = Acc(size)
        so_far = np.zeros(mc.cov_sums(D))
        for R, H in (first, second, first):
            host = mc.data(regime, n, H, R)
            ref = mc.reference_for(regime, host)
            traj = Traj(host.shape, host)
            L = mc.additions(mc.tiling(R, H, mc.MOM_BLOCK, D, False), mc.MOM_BLOCK, D)
            fresh = _standalone(sw, p, D, traj, sw.kernels.cov_acc_doubles(p, R, H))
            _check(key, (n, R, H, regime), fresh, ref, L, regime == "c")
            got = _standalone(sw, p, D, traj, size, acc=acc)
            assert np.array_equal(_bits(got), _bits(so_far + fresh)), (n, R, H, regime)
            so_far = got
    _keep()


def test_statuses_of_sw_traj_moments_f64(sw):
    """Through ctypes, where the Python wrapper would refuse first."""
    from swimmer_amd._lib import load, ptr, stream_ptr
    lib = load()
    p = sw.SwParams.make(3)
    D, R, H = 8, 65, 5
    traj = Traj((H, D, R), mc.data("c", 3, H, R))
    acc = Acc(sw.kernels.cov_acc_doubles(p, R, H), _prefill(D))

    def call(p_, R_, H_, traj_, acc_):
        rc = lib.sw_traj_moments_f64(ctypes.byref(p_) if p_ is not None else None, R_, H_, traj_, acc_, stream_ptr())
        assert np.array_equal(acc.sums(D), _prefill(D)), "acc was touched"
        return rc
    assert call(p, 0, H, ptr(traj.t), ptr(acc.t)) == 0                 # nothing to add: OK, acc untouched
    assert call(p, R, 0, ptr(traj.t), ptr(acc.t)) == 0
    assert call(p, 0, 0, None, None) == 0
    assert call(p, -1, H, ptr(traj.t), ptr(acc.t)) == 3                # SW_ERR_SIZE
    assert call(p, R, -1, ptr(traj.t), ptr(acc.t)) == 3
    assert call(p, R, H, None, ptr(acc.t)) == 1                        # SW_ERR_NULL
    assert call(p, R, H, ptr(traj.t), None) == 1
    assert call(None, R, H, ptr(traj.t), ptr(acc.t)) == 1
    for n in (1, 9):                                                    # SW_ERR_SEGMENTS: n outside 2..8
        bad = sw.SwParams.make(3)
        bad.n = n
        assert call(bad, R, H, ptr(traj.t), ptr(acc.t)) == 2
    bad = sw.SwParams.make(3, l_i=float("nan"))                         # SW_ERR_PARAM
    assert call(bad, R, H, ptr(traj.t), ptr(acc.t)) == 4
    bad = sw.SwParams.make(3, flags=32)
    assert call(bad, R, H, ptr(traj.t), ptr(acc.t)) == 4
    with pytest.raises(sw.SwimmerHipError):
        sw.kernels.cov_acc_doubles(p, -1, 5)
    with pytest.raises(sw.SwimmerHipError):                             # the wrapper: acc one double short
        sw.kernels.traj_moments(p, traj.t, acc.t[:-1])


# ------------------------------------------------------------------------------------------------ owed passes
class Launch(object):
    """The arguments of one ARS rollout launch of the pipeline (capture and V2 moments: the agent's launch) and
    guarded-by-size outputs of its own."""

    def __init__(self, sw, f, n_dir, H):
        n, D, R = f.n, mc.dims(f.n), 2 * n_dir
        rs = mc._rs("owed", f.name, n, n_dir, H)
        self.f, self.n_dir, self.H, self.R, self.D = f, n_dir, H, R, D
        self.p = sw.SwParams.make(n, 0.8, 1.2, 10.2, 1e-3, flags=f.flags)
        self.nu = 0.05
        self.policy = _dev(0.1 * (2 * rs.rand(n - 1, D) - 1))
        self.deltas_host = torch.as_tensor(2 * rs.rand(n_dir, n - 1, D) - 1).pin_memory()
        self.deltas_of_slot = {}      # one device buffer per ring slot, as the pipeline's pacing assumes
        self.deltas = None            # the slot buffer of the latest launch (every one holds deltas_host's bytes)
        self.mean = _dev(0.01 * rs.standard_normal(D))
        self.inv_std = _dev(1.0 + 0.1 * rs.rand(D))
        self.blocks = sw.kernels.moments_blocks(R)

    def outputs(self, traj=True, mom=True):
        return dict(returns=torch.full((self.R,), SENTINEL, dtype=torch.float64, device=DEV),
                    traj=Traj((self.H, self.D, self.R)) if traj else None,
                    moments=torch.full((self.blocks, 2 * self.D), SENTINEL, dtype=torch.float64, device=DEV)
                    if mom else None,
                    status=torch.full((self.R,), -1, dtype=torch.int32, device=DEV))

    def through_pipeline(self, pipe, out, cov_acc, p=None, v2=True):
        slot = pipe.next_slot()
        if slot not in self.deltas_of_slot:
            # torch.empty, not zeros: a fill on this stream could land behind the pipeline's copy on its own stream
            self.deltas_of_slot[slot] = torch.empty(tuple(self.deltas_host.shape), dtype=torch.float64, device=DEV)
        self.deltas = self.deltas_of_slot[slot]
        pipe.rollouts(slot, p or self.p, self.n_dir, 0, self.n_dir, self.H, self.deltas_host, self.deltas,
                      self.policy, self.nu, self.mean if v2 else None, self.inv_std if v2 else None, out["returns"],
                      out["traj"].t if out["traj"] else None, out["moments"], cov_acc, out["status"])

    def without_side_job(self, sw, out, p=None, v2=True):
        sw.kernels.ars_rollouts(p or self.p, self.H, self.policy, self.deltas, self.nu, 0, self.n_dir,
                                mean=self.mean if v2 else None, inv_std=self.inv_std if v2 else None,
                                returns=out["returns"], traj=out["traj"].t if out["traj"] else None,
                                moments=out["moments"], status=out["status"])


def _owed_pass(sw, pipe, la, size, data_dev, ride):
    """launch k with traj_A and cov_acc | traj_A <- data | launch k + 1 with traj_B, or sync_cov  (module docstring)."""
    acc = Acc(size)
    a = la.outputs()
    la.through_pipeline(pipe, a, acc.t)
    a["traj"].t.copy_(data_dev)            # same stream: behind launch k's stores, ahead of the pass
    b = None
    if ride:
        b = la.outputs()
        la.through_pipeline(pipe, b, None)
        torch.cuda.synchronize()           # no flush: the pass has run inside launch k + 1
        got = acc.sums(la.D)
        pipe.sync_cov()                    # nothing is owed any more
        assert np.array_equal(_bits(got), _bits(acc.sums(la.D)))
    else:
        pipe.sync_cov()
        got = acc.sums(la.D)
    assert bool(torch.isnan(a["traj"].whole[:MARGIN]).all()) and bool(torch.isnan(a["traj"].whole[-MARGIN:]).all())
    return got, b, acc


def _owed_case(sw, pipe, f, n_dir, H, regimes):
    D, R = mc.dims(f.n), 2 * n_dir
    la = Launch(sw, f, n_dir, H)
    t = mc.tiling(R, H, f.block, D, True)
    L = mc.additions(t, f.block, D)
    size = sw.kernels.cov_acc_doubles(la.p, R, H)
    assert size == mc.acc_doubles(f.n, R, H) >= mc.cov_sums(D) + 1 + t.n_tiles * (D + D * D)
    name = mc.form_name(D, f.block)
    plain = None
    for regime in regimes:
        host = mc.data(regime, f.n, H, R)
        ref = mc.reference_for(regime, host)
        data_dev = _dev(host)
        what = (mc.riding_id(f), n_dir, H, regime, t.n_tiles)
        flushed, _, acc = _owed_pass(sw, pipe, la, size, data_dev, ride=False)
        if regime == "c":
            acc.check_tiles(D, host, t, what + ("flush",))
        _check("owed/flush_traj_moments_kernel_%s/%s_n%d" % (name, f.name, f.n), what, flushed, ref, L, regime == "c")
        if not f.rides:
            continue
        rode, b, acc = _owed_pass(sw, pipe, la, size, data_dev, ride=True)
        if regime == "c":
            acc.check_tiles(D, host, t, what + ("ride",))
        _check("owed/side_cov_tile_%s/%s_n%d" % (name, f.name, f.n), what, rode, ref, L, regime == "c")
        assert np.array_equal(_bits(rode), _bits(flushed)), (what, "ride against flush")
        if plain is None:         # the rollouts of launch k + 1 are not disturbed by the workgroups behind them
            plain = la.outputs()
            la.without_side_job(sw, plain)
            torch.cuda.synchronize()
        _same_outputs(b, plain, what)


def _same_outputs(b, plain, what):
    for k in ("returns", "moments", "status"):
        assert (b[k] is None and plain[k] is None) or torch.equal(b[k].view(torch.int32), plain[k].view(torch.int32)), \
            (what, k)
    if b["traj"] is not None:
        assert torch.equal(b["traj"].whole.view(torch.int64), plain["traj"].whole.view(torch.int64)), (what, "traj_B")


def carrying_variants(sw, f):
    """(name, traj, moments, v2, flags) of launch k + 1: every (TRAJ, MOM) instantiation of the form's ARS kernel --
    each has its own copy of side_cov_tile behind its rollouts -- and, in the mirror-quad form, the three older
    capture-and-moments kernels that a flag keeps a launch on."""
    L = sw._lib
    out = [("traj_mom", True, True, True, f.flags), ("traj", True, False, False, f.flags),
           ("mom", False, True, True, f.flags), ("none", False, False, False, f.flags)]
    if f.name == "oct3" and not QUAD_ENV:
        out += [("traj_mom_split", True, True, True, L.FLAG_CAPTURE_SPLIT),
                ("traj_mom_packed_v1", True, True, True, L.FLAG_CAPTURE_PACKED_V1),
                ("traj_mom_lean_v1", True, True, True, L.FLAG_CAPTURE_LEAN_V1)]
    return out


FORMS_HERE = tuple(f for f in mc.RIDING_FORMS if f.quad_env == QUAD_ENV)
BIG_HERE = tuple(f for f in FORMS_HERE if (f.name, f.n) in mc.BIG_RIDING)


@pytest.mark.parametrize("f", FORMS_HERE, ids=mc.riding_id)
def test_owed_pass_rides_and_flushes(sw, f):
    """n_dir in {1, 32, 33, 65, 129} (and 31, 63, 127) x H in {1, 2, 5, T - 1, T, T + 1, 2 T + 3}, T the form's
    riding tchunk: one tile, a ragged last column tile, two and three step tiles."""
    pipe = sw.kernels.ArsPipeline()
    try:
        for n_dir, H in mc.riding_shapes(f):
            _owed_case(sw, pipe, f, n_dir, H, mc.REGIMES)
    finally:
        torch.cuda.synchronize()
        pipe.close()
    _keep()


@pytest.mark.parametrize("f", tuple(f for f in FORMS_HERE if f.rides), ids=mc.riding_id)
def test_owed_pass_rides_in_every_rollout_kernel_of_the_form(sw, f):
    """66 rollouts x T + 1 steps (two column tiles, two step tiles), regime c: whichever kernel of the form launch
    k + 1 is, the pass behind its rollouts is exact, tile by tile, and its rollouts are those of the same launch
    through sw_ars_rollouts_f64.

    What this cannot tell: whether the pass rode in launch k + 1 or was flushed in front of it.  Both run behind the
    copy and ahead of the synchronisation, in the same tiling, and leave the same bits in acc and in the scratch rows
    (check_tiles pins the tiling, through the columns per tile, not the kernel that ran it); the library has no call
    that says whether a pass is still owed.  That a launch of the same form and n carries the pass is read off
    sw_ars_iteration_rollouts_f64 (`ride`), not observed here.  The same holds for test_owed_pass_rides_and_flushes,
    and tests/test_cov_matrix_cpu.py's look at rollout_matrix_cases.instantiation_of only says that each form's
    launch names one compiled kernel, not which form the dispatch picks."""
    n_dir, H = 33, mc.riding_T(f) + 1
    D, R = mc.dims(f.n), 2 * n_dir
    la = Launch(sw, f, n_dir, H)
    t = mc.tiling(R, H, f.block, D, True)
    size = sw.kernels.cov_acc_doubles(la.p, R, H)
    host = mc.data("c", f.n, H, R)
    ref, data_dev = mc.reference_exact(host), _dev(host)
    pipe = sw.kernels.ArsPipeline()
    try:
        for name, traj, mom, v2, flags in carrying_variants(sw, f):
            p = sw.SwParams.make(f.n, 0.8, 1.2, 10.2, 1e-3, flags=flags)
            acc, a, b = Acc(size), la.outputs(), la.outputs(traj, mom)
            la.through_pipeline(pipe, a, acc.t)
            a["traj"].t.copy_(data_dev)
            la.through_pipeline(pipe, b, None, p=p, v2=v2)
            got = acc.sums(D)
            what = (mc.riding_id(f), name)
            assert np.array_equal(got, mc.packed(ref)), what
            acc.check_tiles(D, host, t, what)
            plain = la.outputs(traj, mom)
            la.without_side_job(sw, plain, p=p, v2=v2)
            torch.cuda.synchronize()
            _same_outputs(b, plain, what)
            pipe.sync_cov()
    finally:
        torch.cuda.synchronize()
        pipe.close()


@pytest.mark.parametrize("regime", mc.REGIMES)
@pytest.mark.parametrize("f", BIG_HERE, ids=mc.riding_id)
def test_owed_pass_with_more_than_192_tiles(sw, f, regime):
    """The merge's fourth interleaved partial in the form's own instantiation (64, 128 and 256 threads)."""
    n_dir, H = mc.BIG_RIDING[(f.name, f.n)]
    assert mc.tiling(2 * n_dir, H, f.block, mc.dims(f.n), True).n_tiles > 192
    pipe = sw.kernels.ArsPipeline()
    try:
        _owed_case(sw, pipe, f, n_dir, H, (regime,))
    finally:
        torch.cuda.synchronize()
        pipe.close()
    _keep()


def test_quad3_picked_by_the_dispatch_side_cov_tile_D8_B64_wide(sw):
    """8194 rollouts: beyond the mirror-quad form's 8192, so the launches are the quad form's in any process, and the
    owed block is its 64 threads (the accumulator's size and the bound are those of that tiling)."""
    f = [x for x in mc.RIDING_FORMS if x.name == "quad3"][0]
    n_dir, H = mc.QUAD_NATURAL
    assert 2 * n_dir > 8192
    pipe = sw.kernels.ArsPipeline()
    try:
        _owed_case(sw, pipe, f, n_dir, H, mc.REGIMES)
    finally:
        torch.cuda.synchronize()
        pipe.close()
    _keep()


def test_quad3_side_cov_tile_D8_B64_wide_and_its_flush_in_a_child_process(tmp_path):
    """rollout_quad3_kernel takes batches this small only with SWIMMER_N3_KERNEL=quad, read once per process: the owed
    passes of the quad form (side_cov_tile<8, 64>, traj_moments_kernel<8, 64>) in a fresh child, whose observed
    figures join this process's record."""
    if QUAD_ENV:          # this process is that child
        return
    env = dict(os.environ, SWIMMER_N3_KERNEL="quad", SWIMMER_REPORT_DIR=str(tmp_path))   # the child reports there
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-s",
                          "-k", "test_owed_pass"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert re.search(r"(?m)^5 passed\b", out.stdout), out.stdout[-2000:]      # both owed-pass tests, the big one x 3
    with open(os.path.join(str(tmp_path), "cov_matrix_quad.json")) as fh:
        for k, v in json.load(fh).items():
            _note(k, v)
    _keep()
