"""The ARS update family (ars_update_kernel, ars_update_multi_kernel, ars_update_counted_kernel at both workgroup
sizes, ars_pack_admitted_kernel) against the long-double restatement of tests/update_matrix_cases.py, at every path of
csrc/swimmer_update.inc (tests/test_update_matrix_cpu.py checks that the cases reach the paths and would show the
mistakes they are there for).

Within the per-case forward-error bounds: policy, sigma_out, running, mean and inv_std of sw_ars_update_f64 and of
sw_ars_update_gathered_f64 at every world size.  Bit for bit: a second call with the same inputs; the gathered call
against the plain one where the shards are row-aligned; sw_ars_update_multi_f64 and sw_ars_update_multi_counted_f64
agent by agent against the single call.  Exact: count, order and packed of sw_ars_pack_admitted_f64.  Every output
buffer sits between two canary margins, and what the contract leaves alone keeps its fill.  The largest ratio
|got - reference| / bound of every path is kept through conftest.observed (profiles/update_matrix_observed.json).
"""
import numpy as np
import pytest
import torch

from conftest import observed

import update_matrix_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 67                    # elements in front of and behind every output buffer
CANARY = -1234567              # a fixed odd value, exact in float64 and in int32
FILL = 777.0                   # of entries that a call must leave alone
_seen = {}


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


class Guarded(object):
    """An output buffer between two margins of CANARY: .t is the tensor the kernel is given."""

    def __init__(self, data=None, shape=None, dtype=torch.float64, fill=0):
        if data is not None:
            data = torch.as_tensor(np.ascontiguousarray(data))
            shape, dtype = tuple(data.shape), data.dtype
        self.numel = int(np.prod(shape))
        self.whole = torch.full((self.numel + 2 * MARGIN,), CANARY, dtype=dtype, device=DEV)
        self.t = self.whole[MARGIN:MARGIN + self.numel].view(shape)
        if data is not None:
            self.t.copy_(data)
        else:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.whole[:MARGIN] == CANARY).all()) and bool((self.whole[MARGIN + self.numel:] == CANARY).all())

    def np(self):
        return self.t.cpu().numpy().copy()


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _note(key, r):
    _seen[key] = max(_seen.get(key, 0.0), r)


def _keep():
    observed("update_matrix", dict(sorted(_seen.items())))


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int64).copy() for a in arrays]


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(_bits(*a), _bits(*b))):
        assert np.array_equal(x, y), (what, i)


def _check(key, what, got, ref):
    """got within the bound of ref, every entry; the ratio is kept before it is asserted."""
    worst = 0.0
    for name, g in got.items():
        r = mc.ratio(g, ref[name])
        _note(f"{key}/{name}", r)
        worst = max(worst, r)
        if not r <= 1.0:
            _keep()
        assert r <= 1.0, (what, name, r)
    return worst


def _single(sw, n, inp_dev, policy0, alpha, b, top_b, v2=None, sigma=True):
    """One sw_ars_update_f64 call into guarded buffers.  v2 = (moments, running: Guarded, n_new) or None: then mean and
    inv_std are passed all the same and must keep their fill.  -> (policy, sigma or None, mean, inv_std) as numpy."""
    d = mc.dims(n)[0]
    p = sw.SwParams.make(n)
    returns, deltas = inp_dev
    pol = Guarded(policy0)
    sig = Guarded(shape=(1,), fill=FILL) if sigma else None
    mean, inv = Guarded(shape=(d,), fill=FILL), Guarded(shape=(d,), fill=FILL)
    kw = {}
    if v2 is not None:
        kw = dict(moments=v2[0], running=v2[1].t, n_new_states=v2[2])
    sw.kernels.ars_update(p, returns, deltas, pol.t, alpha, b, top_b, mean=mean.t, inv_std=inv.t,
                          sigma_out=None if sig is None else sig.t, **kw)
    torch.cuda.synchronize()
    for g in (pol, sig, mean, inv) + ((v2[1],) if v2 is not None else ()):
        assert g is None or g.intact()
    if v2 is None:
        assert (mean.np() == FILL).all() and (inv.np() == FILL).all()
    return pol.np(), None if sig is None else sig.np(), mean.np(), inv.np()


@pytest.mark.parametrize("n", mc.NS)
def test_update_matrix_policy_step_at_every_path(sw, n):
    """sw_ars_update_f64 without `running` over the n_dir x top_b list of the shape: policy and sigma within the
    bounds; the same bits from a second call; mean / inv_std that happen to be passed are untouched; NULL sigma_out."""
    for n_dir in mc.n_dirs(n):
        inp = mc.inputs(n, n_dir)
        on_dev = (_dev(inp["returns"]), _dev(inp["deltas"]))
        for top_b in mc.top_bs(n_dir):
            ref = mc.reference_update(inp["returns"], inp["deltas"], inp["policy"], inp["alpha"], inp["b"], top_b)
            first = _single(sw, n, on_dev, inp["policy"], inp["alpha"], inp["b"], top_b)
            key = "update/%d/%s/%s" % mc.path(n_dir, top_b)
            _check(key, (n, n_dir, top_b), {"policy": first[0], "sigma": first[1][0]}, ref)
            again = _single(sw, n, on_dev, inp["policy"], inp["alpha"], inp["b"], top_b, sigma=top_b != n_dir + 7)
            _same_bits(first[:1], again[:1], (n, n_dir, top_b))
            if again[1] is not None:
                _same_bits(first[1:2], again[1:2], (n, n_dir, top_b, "sigma"))
    _keep()


def _run_sequence(sw, n, n_dir, batches, top_bs):
    """Successive V2 updates on one `running` (from zeros): [(policy, sigma, mean, inv_std, running)] per update."""
    inp = mc.inputs(n, n_dir)
    on_dev = (_dev(inp["returns"]), _dev(inp["deltas"]))
    running = Guarded(shape=(1 + 2 * mc.dims(n)[0],), fill=0)
    out = []
    for bt, top_b in zip(batches, top_bs):
        res = _single(sw, n, on_dev, inp["policy"], inp["alpha"], inp["b"], top_b,
                      v2=(_dev(bt["rows"]), running, bt["n_new"]))
        out.append(res + (running.np(),))
    return out


@pytest.mark.parametrize("n", mc.NS)
def test_update_matrix_merge_at_every_row_count(sw, n):
    """The merging workgroup at both sizes, rows in {1, G - 1, G, G + 1, 8 G, 8 G + 1}: three successive updates on one
    `running` (n0 = 0, then n0 > 0, batch means apart, another n_new) against the list of all states so far."""
    for n_dir in (5, 1025):
        inp = mc.inputs(n, n_dir)
        top_bs = mc.moment_top_bs(n_dir)
        for rows in mc.moment_rows(n, mc.block_of(n_dir)):
            batches, refs = mc.moment_case(n, n_dir, rows)
            got = _run_sequence(sw, n, n_dir, batches, top_bs)
            key = "merge/%d/%s" % mc.merge_path(n, n_dir, rows)
            for u, (pol, sig, mean, inv, run) in enumerate(got):
                assert run[0] == sum(b["n_new"] for b in batches[:u + 1])
                _check(key, (n, n_dir, rows, u), {"running": run, "mean": mean, "inv_std": inv}, refs[u])
                ref = mc.reference_update(inp["returns"], inp["deltas"], inp["policy"], inp["alpha"], inp["b"],
                                          top_bs[u])
                _check("update/%d/%s/%s" % mc.path(n_dir, top_bs[u]), (n, n_dir, rows, u, "step"),
                       {"policy": pol, "sigma": sig[0]}, ref)
            again = _run_sequence(sw, n, n_dir, batches, top_bs)
            for u in range(3):
                _same_bits(got[u], again[u], (n, n_dir, rows, u))
    _keep()


def _run_gathered(sw, n, n_dir, world, top_b):
    d = mc.dims(n)[0]
    p = sw.SwParams.make(n)
    inp = mc.inputs(n, n_dir)
    c = mc.gathered_case(n, n_dir, world)
    deltas = _dev(inp["deltas"])
    running = Guarded(shape=(1 + 2 * d,), fill=0)
    out = []
    for u, bt in enumerate(c["batches"]):
        pol, sig = Guarded(inp["policy"]), Guarded(shape=(1,), fill=FILL)
        mean, inv = Guarded(shape=(d,), fill=FILL), Guarded(shape=(d,), fill=FILL)
        sw.kernels.ars_update_gathered(p, n_dir, _dev(c["buffers"][u]), world, c["chunk"], c["rows_chunk"], deltas,
                                       pol.t, inp["alpha"], inp["b"], top_b, running=running.t,
                                       n_new_states=bt["n_new"], mean=mean.t, inv_std=inv.t, sigma_out=sig.t)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (pol, sig, mean, inv, running))
        out.append((pol.np(), sig.np(), mean.np(), inv.np(), running.np()))
    return out


@pytest.mark.parametrize("n", mc.GATHERED_NS)
def test_update_matrix_gathered_layout_at_every_world(sw, n):
    """sw_ars_update_gathered_f64, world in {1, 2, 3, 8}: ragged last chunks with poisoned slots and zero padding rows
    within the bounds; row-aligned shards (and world = 1) the bits of the plain call on the same data."""
    for n_dir in mc.GATHERED_N_DIRS + mc.GATHERED_ALIGNED:
        inp = mc.inputs(n, n_dir)
        top_b = n_dir // 3
        ref = mc.reference_update(inp["returns"], inp["deltas"], inp["policy"], inp["alpha"], inp["b"], top_b)
        plain = _run_sequence(sw, n, n_dir, mc.gathered_case(n, n_dir, 1)["batches"], (top_b, top_b))
        for world in mc.GATHERED_WORLDS:
            c = mc.gathered_case(n, n_dir, world)
            got = _run_gathered(sw, n, n_dir, world, top_b)
            for u, (pol, sig, mean, inv, run) in enumerate(got):
                what = (n, n_dir, world, u)
                _check(f"gathered/world{world}", what, {"policy": pol, "sigma": sig[0]}, ref)
                _check(f"gathered/world{world}", what, {"running": run, "mean": mean, "inv_std": inv}, c["refs_v2"][u])
                if world == 1 or mc.row_aligned(n_dir, world):
                    _same_bits(got[u], plain[u], what)
                else:       # the policy step's order of summation depends on n_dir only, however the shards are cut
                    _same_bits(got[u][:2], plain[u][:2], what)
    _keep()


@pytest.mark.parametrize("v2", (False, True), ids=("v1", "v2"))
@pytest.mark.parametrize("n", mc.NS)
def test_update_matrix_multi_is_the_single_call_per_agent(sw, n, v2):
    """sw_ars_update_multi_f64, three agents with unrelated data at both workgroup sizes: every agent's outputs have the
    bits of sw_ars_update_f64 on its slices (which are within the bounds of the reference); two successive updates."""
    d = mc.dims(n)[0]
    S = mc.MULTI_AGENTS
    p = sw.SwParams.make(n)
    for n_dir in mc.MULTI_N_DIRS:
        c = mc.multi_case(n, n_dir)
        ag, top_b = c["agents"], c["top_b"]
        returns, deltas = _dev(np.stack([a["returns"] for a in ag])), _dev(np.stack([a["deltas"] for a in ag]))
        running = Guarded(shape=(S, 1 + 2 * d), fill=0)
        singles = [Guarded(shape=(1 + 2 * d,), fill=0) for _ in range(S)]
        for u in range(2 if v2 else 1):
            pol, sig = Guarded(np.stack([a["policy"] for a in ag])), Guarded(shape=(S,), fill=FILL)
            mean, inv = Guarded(shape=(S, d), fill=FILL), Guarded(shape=(S, d), fill=FILL)
            kw = {}
            if v2:
                kw = dict(moments=_dev(np.stack([b[u]["rows"] for b in c["batches"]])), running=running.t,
                          n_new_states=c["batches"][0][u]["n_new"])
                assert all(b[u]["rows"].shape == c["batches"][0][u]["rows"].shape for b in c["batches"])
                assert len({b[u]["n_new"] for b in c["batches"]}) == 1          # a launch has one n_new_states
            sw.kernels.ars_update_multi(p, returns, deltas, pol.t, ag[0]["alpha"], ag[0]["b"], top_b, mean=mean.t,
                                        inv_std=inv.t, sigma_out=sig.t, **kw)
            torch.cuda.synchronize()
            assert all(g.intact() for g in (pol, sig, mean, inv, running))
            if not v2:
                assert (mean.np() == FILL).all() and (inv.np() == FILL).all() and not running.np().any()
            for a in range(S):
                one = _single(sw, n, (returns[a], deltas[a]), ag[a]["policy"], ag[0]["alpha"], ag[0]["b"], top_b,
                              v2=(kw["moments"][a], singles[a], kw["n_new_states"]) if v2 else None)
                _same_bits((pol.np()[a], sig.np()[a:a + 1], mean.np()[a], inv.np()[a]), one, (n, n_dir, u, a))
                if v2:
                    _same_bits((running.np()[a],), (singles[a].np(),), (n, n_dir, u, a, "running"))
                ref = mc.reference_update(ag[a]["returns"], ag[a]["deltas"], ag[a]["policy"], ag[0]["alpha"],
                                          ag[0]["b"], top_b)
                _check("multi/%d" % mc.block_of(n_dir), (n, n_dir, u, a), {"policy": pol.np()[a], "sigma": sig.np()[a]},
                       ref)
                if v2:
                    _check("multi/%d" % mc.block_of(n_dir), (n, n_dir, u, a),
                           {"running": running.np()[a], "mean": mean.np()[a], "inv_std": inv.np()[a]},
                           c["refs_v2"][a][u])
    _keep()


@pytest.mark.parametrize("v2", (False, True), ids=("v1", "v2"))
@pytest.mark.parametrize("top_b_max", mc.COUNTED_TOP_B)
@pytest.mark.parametrize("n", mc.COUNTED_NS)
def test_update_matrix_counted_is_the_single_call_per_count(sw, n, top_b_max, v2):
    """sw_ars_update_multi_counted_f64 with counts on both sides of the workgroup-size switch (both sizes launch, each
    serves its agents): agent a has the bits of sw_ars_update_f64 with n_dir = count, top_b = min(top_b_max, count),
    n_new_states = 2 count H and the first ceil(2 count / 16) rows; the agents with count 0 and -3 keep every fill."""
    d = mc.dims(n)[0]
    S, N, H = len(mc.COUNTS), mc.COUNTED_MAX, mc.COUNTED_H
    p = sw.SwParams.make(n)
    c = mc.counted_case(n)
    returns, deltas, moments = _dev(c["returns"]), _dev(c["deltas"]), _dev(c["moments"])
    count = torch.as_tensor(np.array(mc.COUNTS, dtype=np.int32), device=DEV)
    pol, sig = Guarded(c["policy"]), Guarded(shape=(S,), fill=FILL)
    mean, inv, running = Guarded(shape=(S, d), fill=FILL), Guarded(shape=(S, d), fill=FILL), Guarded(c["running"])
    kw = dict(moments=moments, running=running.t) if v2 else {}
    sw.kernels.ars_update_multi_counted(p, H, count, returns, deltas, pol.t, c["alpha"], c["b"], top_b_max, mean=mean.t,
                                        inv_std=inv.t, sigma_out=sig.t, **kw)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (pol, sig, mean, inv, running))
    served = 0
    for a, cnt in enumerate(mc.COUNTS):
        k = mc.counted_n_dir(cnt)
        got = (pol.np()[a], sig.np()[a:a + 1], mean.np()[a], inv.np()[a], running.np()[a])
        if k == 0 or not v2:
            _same_bits(got[2:], (np.full(d, FILL), np.full(d, FILL), c["running"][a]), (n, a, "left alone"))
        if k == 0:
            _same_bits(got[:2], (c["policy"][a], np.full(1, FILL)), (n, a, "left alone"))
            continue
        served += 1
        one_running = Guarded(c["running"][a])
        one = _single(sw, n, (returns[a, :2 * k].contiguous(), deltas[a, :k].contiguous()), c["policy"][a], c["alpha"],
                      c["b"], min(top_b_max, k),
                      v2=(moments[a, :mc.rows_of(k)].contiguous(), one_running, 2 * k * H) if v2 else None)
        _same_bits(got[:4], one, (n, a, cnt))
        _same_bits(got[4:], (one_running.np(),), (n, a, cnt, "running"))
        assert np.isfinite(np.concatenate([x.ravel() for x in got])).all()
    assert served == 5


@pytest.mark.parametrize("n_dir", mc.PACK_N_DIRS)
@pytest.mark.parametrize("n", mc.PACK_NS)
def test_update_matrix_pack_admitted_is_exact(sw, n, n_dir):
    """sw_ars_pack_admitted_f64: count, order (ascending, then -1) and packed equal the reference exactly for every flag
    pattern, with and without a status array; packed rows from count on keep their fill."""
    p = sw.SwParams.make(n)
    for name in mc.PACK_PATTERNS:
        for with_status in (False, True):
            c = mc.pack_case(n, n_dir, name, with_status)
            want_count, want_order, want_packed = mc.reference_pack(c["admit"], c["status"], c["deltas"])
            count = Guarded(shape=(mc.PACK_AGENTS,), dtype=torch.int32, fill=-7)
            order = Guarded(shape=c["admit"].shape, dtype=torch.int32, fill=-7)
            packed = Guarded(shape=c["deltas"].shape, fill=FILL)
            sw.kernels.ars_pack_admitted(p, _dev(c["admit"]), _dev(c["deltas"]),
                                         status=None if c["status"] is None else _dev(c["status"]), count=count.t,
                                         order=order.t, packed=packed.t)
            torch.cuda.synchronize()
            what = (n, n_dir, name, with_status)
            assert count.intact() and order.intact() and packed.intact(), what
            assert np.array_equal(count.np(), want_count), what
            assert np.array_equal(order.np(), want_order), what
            want = np.where(np.isnan(want_packed), FILL, want_packed)
            assert np.array_equal(packed.np(), want), what
