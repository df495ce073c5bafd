"""Every compiled instantiation of the single-agent rollout kernels (sw_rollout_f64, sw_ars_rollouts_f64: the 88 of
tests/rollout_matrix_cases.py INSTANTIATIONS) against oracle.swimmer_oracle -- the twin model's 14,
rollout_kernel<N, ARS, true>, against oracle.twin_step stepped from Python.  This file is the ROOT of the suite's
tree of bit-equalities: the multi-agent, gate, counted and safe-batch tests compare their kernels with these launches,
so a wrong instantiation here is one they would agree with.  tests/test_rollout_matrix_cpu.py checks that the list is
what the library holds and that the cases exercise what is compared here.

One case per (form, n, entry point); the n = 3 cases run once more on the quad kernel in a child process
(SWIMMER_N3_KERNEL=quad is read once per process).  In each case, for V1 and V2 and every edge shape of the cases
module, every (TRAJ, MOM) combination the form has is launched through the C ABI with guards around every output: a
trajectory of H + 1 slabs, moments with one extra row, returns / status / final_state with 16 extra cells, all
pre-filled with a sentinel.

For every launch: every cell that should be written is written and every guard untouched; status 0; returns, the whole
trajectory and final_state within 1e-9 max(1, |ref|) of the oracle (the project's bound for runs of up to 1000 steps);
final_state the bits of the last trajectory slab; EVERY MOMENT ROW on its own (row b: rollouts 16 b .. 16 b + 15, the
valid ones only) within 1e-9 of the row's sum of absolute terms.  That sum is taken over the row's columns, once for
the sums of obs - c and once for the sums of squares: an entry's OWN terms can be pure rounding residue -- from rest
(every ARS launch, every plain one without start states) Gdot is physically zero after the first step, 8e-19 in the
oracle and another residue or 0 in a kernel, 1e-10 after 4 steps and 5e-8 after 13 -- and no kernel can agree with the
oracle to nine digits of a residue.  Per entry the worst figure is only recorded (moment_entry_observed; first run:
1.0 to 2.2 in every case with launches from rest, 4e-14 .. 7e-13 in the loop-crossing cases against 2e-16 .. 1e-15
of their rows).  A row in the wrong block, or a rollout counted in the neighbouring row, is off by a whole rollout's
terms: ~ 1 / 16 of the scale, 1e7 times the bound.

Across the launches of one shape: returns, status, final_state and whichever of trajectory / moments two launches both
produce are bit-identical -- the records do not enter the step's arithmetic (first run: no pair differed).

The loop-crossing cases (n = 4..8; the cases module says what they hold) run with trajectory and moments and with
neither, through the plain entry point with their start states and through the ARS one from rest, same bounds.

The worst figures of every case go to observed("rollout_matrix", ...), the child's to "rollout_matrix_quad";
profiles/rollout_matrix_observed.json and rollout_matrix_quad_observed.json hold those of the first run (7008 + 708
launches: trajectory <= 1.5e-14, returns <= 2.8e-14, moment rows <= 1.3e-13, no pair with different bits).

THE TWIN CASES (form "twin", n = 2..8: rollout_kernel<N, ARS, true>, the lane form's shapes and variants, all of
them) are the root for everything that is compared bit for bit with twin launches: ars_multi_lane_kernel<N, true> in
tests/test_ars_multi_gpu.py and the twin forms of the gate, counted and ensemble tests.  Same checks, same bound.  From
the twin's 0.001 start the returns are ~ 1e-3, not a residue, and every moment entry has terms of its own: the per-entry
figure is small here too.  profiles/rollout_matrix_twin_observed.json holds the twin cases' figures of their first run
(3920 launches: trajectory <= 6.9e-15, returns <= 1.2e-15, final_state <= 3.6e-15, moment rows <= 6.1e-16, moment
entries <= 1.7e-13, no pair with different bits).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import observed

import rollout_matrix_cases as mc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 16                                                          # cells behind returns / status / final_state
QUAD_ENV = os.environ.get("SWIMMER_N3_KERNEL", "")[:1] == "q"       # this process runs n = 3 on the quad kernel
_seen = {}


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return swimmer_amd


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda:0")


def filled(n, value=SENTINEL, dtype=torch.float64):
    return torch.full((n,), value, dtype=dtype, device="cuda:0")


def upload(inp):
    """A launch's inputs on the device, once for all its variants."""
    ars = "deltas" in inp and inp.get("as_ars", True)
    out = dict(mean=dev(inp["mean"]), inv_std=dev(None if inp["var"] is None else inp["var"] ** -0.5))
    if ars:
        out.update(policy=dev(inp["policy"]), deltas=dev(inp["deltas"]))
    else:
        out.update(policies=dev(inp["policies"]), state0=dev(None if inp["state0"] is None else inp["state0"].T))
    return ars, out


def launch(sw, inp, on_dev, ars, want_traj, want_mom, flags):
    """One launch through the C ABI, every output guarded: dict of host arrays."""
    from swimmer_amd._lib import check, load, ptr, stream_ptr
    n, H = inp["n"], inp["H"]
    d, R = 2 * n + 2, inp["policies"].shape[0]
    B = (R + mc.MOM_GROUP - 1) // mc.MOM_GROUP
    p = sw.SwParams.make(n, *mc.model_params(inp.get("model", "gym")), flags=flags)
    ret, status = filled(R + GUARD), filled(R + GUARD, -1, torch.int32)
    traj = filled((H + 1) * d * R) if want_traj else None
    mom = filled((B + 1) * 2 * d) if want_mom else None
    fin = None
    if ars:
        check(load().sw_ars_rollouts_f64(ctypes.byref(p), inp["dir_begin"], inp["n_dir"], H, ptr(on_dev["policy"]),
                                         ptr(on_dev["deltas"]), inp["nu"], ptr(on_dev["mean"]), ptr(on_dev["inv_std"]),
                                         ptr(ret), ptr(traj), ptr(mom), ptr(status), stream_ptr()),
              "sw_ars_rollouts_f64")
    else:
        fin = filled(d * R + GUARD)
        check(load().sw_rollout_f64(ctypes.byref(p), R, H, ptr(on_dev["policies"]), ptr(on_dev["mean"]),
                                    ptr(on_dev["inv_std"]), ptr(on_dev["state0"]), ptr(ret), ptr(traj), ptr(fin),
                                    ptr(mom), ptr(status), stream_ptr()), "sw_rollout_f64")
    torch.cuda.synchronize()
    out = dict(returns=ret[:R].cpu().numpy(), returns_guard=ret[R:].cpu().numpy(),
               status=status[:R].cpu().numpy(), status_guard=status[R:].cpu().numpy())
    if traj is not None:
        t = traj.cpu().numpy().reshape(H + 1, d, R)
        out.update(traj=t[:H].transpose(2, 0, 1), traj_guard=t[H])            # [R, H, d] as the oracle's
    if mom is not None:
        m = mom.cpu().numpy().reshape(B + 1, 2 * d)
        out.update(moments=m[:B], moments_guard=m[B])
    if fin is not None:
        f = fin.cpu().numpy()
        out.update(final=f[:d * R].reshape(d, R).T, final_guard=f[d * R:])     # [R, d]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


class Figures:
    """The worst figures of a case, and what went wrong in it."""

    def __init__(self):
        self.fig = dict(trajectory=0.0, returns=0.0, final_state=0.0, moment_row=0.0, moment_entry_observed=0.0,
                        bit_different_pairs=0, launches=0)
        self.failures = []

    def worse(self, key, value, bound, what):
        value = float(value)
        self.fig[key] = value if value != value else max(self.fig[key], value)      # a NaN figure stays
        if not value <= bound:
            self.failures.append((what, key, value))

    def require(self, ok, what):
        if not ok:
            self.failures.append(what)


def rel(got, ref):
    """The error in units of max(1, |ref|), NaN if anything is."""
    if got.size == 0:
        return 0.0
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float("nan") if np.isnan(e).any() else e.max()


def check_launch(F, out, ref, what):
    F.fig["launches"] += 1
    for key in out:
        if key.endswith("_guard"):
            F.require((out[key] == (-1 if key == "status_guard" else SENTINEL)).all(), (what, key, "was written"))
    F.require(not (out["returns"] == SENTINEL).any(), (what, "a return was not written"))
    F.require(not out["status"].any(), (what, "status", out["status"].tolist()))
    F.worse("returns", rel(out["returns"], ref["returns"]), mc.TOL, what)
    if "traj" in out:
        F.require(not (out["traj"] == SENTINEL).any(), (what, "a trajectory cell was not written"))
        F.worse("trajectory", rel(out["traj"], ref["traj"]), mc.TOL, what)
    if "final" in out:
        F.require(not (out["final"] == SENTINEL).any(), (what, "a final_state cell was not written"))
        F.worse("final_state", rel(out["final"], ref["final"]), mc.TOL, what)
        if "traj" in out and out["traj"].shape[1]:
            F.require(np.array_equal(bits(out["final"]), bits(out["traj"][:, -1])),
                      (what, "final_state is not the last trajectory slab"))
    if "moments" in out:
        rows, terms = mc.moment_rows(ref["traj"])
        d = rows.shape[1] // 2
        F.require(not (out["moments"] == SENTINEL).any(), (what, "a moment cell was not written"))
        err = np.abs(out["moments"] - rows)
        for half in (slice(0, d), slice(d, 2 * d)):               # the sums of obs - c, the sums of its square
            worst, scale = err[:, half].max(axis=1), terms[:, half].sum(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                figure = np.where(scale > 0, worst / scale, np.where(worst == 0, 0.0, np.inf))
            F.worse("moment_row", float("nan") if np.isnan(err).any() else figure.max(), mc.TOL, what)
        with np.errstate(invalid="ignore", divide="ignore"):      # observed only: every entry against its own terms
            entry = np.where(terms > 0, err / terms, 0.0)
        F.fig["moment_entry_observed"] = max(F.fig["moment_entry_observed"], float(np.nan_to_num(entry, nan=np.inf).max()))


def check_same_bits(F, outs, what):
    """Across the launches of one shape: whatever two launches both produce is bit-identical."""
    names = list(outs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for key in ("returns", "status", "final", "traj", "moments"):
                if key in outs[a] and key in outs[b] and not np.array_equal(bits(outs[a][key]), bits(outs[b][key])):
                    F.fig["bit_different_pairs"] += 1
                    F.failures.append((what, key, a, "and", b, "differ in their bits"))


def run_shape(sw, F, form, inp, what, variants=None):
    ars, on_dev = upload(inp)
    ref = mc.reference(inp)
    outs = {}
    for name, traj, mom, flags in (variants or mc.variants(form)):
        mc.instantiation_of(form, inp["n"], ars, traj, mom, flags, QUAD_ENV)      # the launch is one of the list's
        outs[name] = launch(sw, inp, on_dev, ars, traj, mom, flags)
        check_launch(F, outs[name], ref, what + (name,))
    check_same_bits(F, outs, what)


def finish(F, name):
    _seen[name] = F.fig
    observed("rollout_matrix_quad" if QUAD_ENV else "rollout_matrix", _seen)
    for f in F.failures:
        print("failed check:", f)
    assert not F.failures, (len(F.failures), F.failures[:8], F.fig)
    assert F.fig["launches"] > 0


@pytest.mark.parametrize("entry", ("plain", "ars"))
@pytest.mark.parametrize("form,n", mc.FORMS)
def test_every_instantiation_against_the_oracle(sw, form, n, entry):
    F, model = Figures(), mc.model_of(form)
    for v2 in (False, True):
        if entry == "plain":
            for H, R, s0 in mc.plain_shapes(form):
                run_shape(sw, F, form, mc.plain_inputs(n, H, R, s0, v2, model),
                          ("H", H, "R", R, "state0", s0, "v2", v2))
        else:
            for H, n_dir, dir_begin in mc.ars_shapes(form):
                run_shape(sw, F, form, mc.ars_inputs(n, H, n_dir, dir_begin, v2, model),
                          ("H", H, "n_dir", n_dir, "dir_begin", dir_begin, "v2", v2))
    finish(F, f"{form}_n{n}_{entry}")


@pytest.mark.parametrize("n", sorted(mc.CROSSING))
def test_waves_that_cross_between_the_unchecked_and_the_checked_loop(sw, n):
    """Trajectory stores (soff) and the moment accumulators live across both loops, in waves that change loops at
    steps that are no multiple of four, with and without an ARS prologue."""
    F = Figures()
    variants = [v for v in mc.variants("row") if v[0] in ("none", "traj_mom")]
    plain = dict(mc.crossing_case(n), as_ars=False)
    run_shape(sw, F, "row", plain, ("crossing", "plain"), variants)
    run_shape(sw, F, "row", mc.crossing_case(n, from_rest=True), ("crossing", "ars"), variants)
    finish(F, f"crossing_n{n}")


def test_the_n3_cases_on_the_quad_kernel_in_a_child_process():
    """rollout_quad3_kernel<ARS, TRAJ, MOM> takes batches this small only with SWIMMER_N3_KERNEL=quad, which the
    library reads once per process: the n = 3 segment-per-lane cases of this file once more, in a fresh child."""
    if QUAD_ENV:      # this process already runs them there (and the child's -k never selects this test)
        return
    env = dict(os.environ, SWIMMER_N3_KERNEL="quad")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-s",
                          "-k", "test_every_instantiation_against_the_oracle and oct3"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "2 passed" in out.stdout
