"""tests/cov_matrix_cases.py on its own, without a GPU: the restated tiling against sw_cov_acc_doubles (pure host
arithmetic of the library, the only pin on the cap of 4096 tiles where it binds on ny: reaching that on the GPU takes
gigabytes of trajectory), the case list of tests/test_cov_matrix_gpu.py against what it is there to reach, the exact
reference of regime c against the long-double one, and the derived bound against the mistakes it must show."""
import ctypes

import numpy as np
import pytest

import cov_matrix_cases as mc


@pytest.fixture(scope="module")
def sw():
    import swimmer_amd
    swimmer_amd._lib.load()
    return swimmer_amd


def test_the_covariance_knobs_are_not_set():
    assert not mc.knobs_set(), (
        "%s set in the environment: the library reads it once per process and it changes the covariance tiling "
        "(or pacing) these tests restate -- unset it" % ", ".join(mc.knobs_set()))


def test_long_double_is_the_x87_format():
    assert np.finfo(np.longdouble).eps == 2.0 ** -63, "the reference needs a 64-bit significand"


SWEEP_R = (1, 63, 64, 65, 255, 256, 257, 4096, 8192, 16384, 262144, 262145, 1048577)
SWEEP_H = (1, 2, 7, 8, 9, 31, 32, 33, 127, 128, 129, 1000, 2049, 4097, 8193)


def test_tiling_reproduces_sw_cov_acc_doubles(sw):
    """n = 2..8 x SWEEP_R x SWEEP_H: the restated cov_tiling, maximised over the four owed blocks and both `riding`
    values, gives the library's figure.  The 128-thread block is only ever owed at n = 3 (the mirror-quad form);
    the library maximises over it for every n, which asks for no more scratch anywhere in the sweep."""
    assert not mc.knobs_set()
    lib = sw._lib.load()
    cap_on_nbx = cap_on_ny = 0
    for n in mc.NS:
        p = sw.SwParams.make(n)
        D = mc.dims(n)
        for R in SWEEP_R:
            for H in SWEEP_H:
                got = int(lib.sw_cov_acc_doubles(ctypes.byref(p), R, H))
                assert got == mc.acc_doubles(n, R, H), (n, R, H)
                if n != 3:
                    assert got == mc.acc_doubles(n, R, H, blocks=(64, 256)), (n, R, H)
                for block in set(mc.OWED_BLOCKS):
                    for riding in (False, True):
                        t = mc.tiling(R, H, block, D, riding)
                        assert sum(t.lengths) == H and len(t.lengths) == t.ny and max(t.lengths) == t.tchunk
                        assert min(t.lengths) >= 1 and t.nbx * t.cols >= R > (t.nbx - 1) * t.cols
                        assert t.nbx > mc.MAX_TILES or t.n_tiles <= mc.MAX_TILES
                        if t.nbx > mc.MAX_TILES:
                            assert t.ny == 1
                            cap_on_nbx += 1
                        elif riding and t.ny < -(-H // (128 if block < 256 or mc.cov_split(D, block) else 32)):
                            cap_on_ny += 1
    assert cap_on_nbx > 0 and cap_on_ny > 0
    # empty passes: the sums and the ticket only
    p = sw.SwParams.make(4)
    assert int(lib.sw_cov_acc_doubles(ctypes.byref(p), 0, 9)) == mc.cov_sums(10) + 1 == mc.acc_doubles(4, 0, 9)
    assert int(lib.sw_cov_acc_doubles(ctypes.byref(p), 9, 0)) == mc.cov_sums(10) + 1


def test_sw_cov_acc_doubles_refuses_bad_arguments(sw):
    lib = sw._lib.load()
    ok = sw.SwParams.make(3)
    assert int(lib.sw_cov_acc_doubles(ctypes.byref(ok), -1, 5)) == -1
    assert int(lib.sw_cov_acc_doubles(ctypes.byref(ok), 5, -1)) == -1
    for n in (1, 9, 0, -3):
        bad = sw.SwParams.make(3)
        bad.n = n
        assert int(lib.sw_cov_acc_doubles(ctypes.byref(bad), 5, 5)) == -1
    assert int(lib.sw_cov_acc_doubles(None, 5, 5)) == -1


def test_the_tilings_named_in_the_kernels_comments():
    """Fixed points of the restatement, by hand from cov_tiling: riding bases 128 / 32 / 128, the standalone
    want / target / floor-of-8 rule, and the issue's merge example."""
    assert mc.tiling(2112, 769, 64, 8, True)[1:4] == (33, 7, 110)            # 64-thread tiles: base 128
    assert mc.tiling(16, 1000, 128, 8, True)[1:4] == (1, 8, 125)
    assert mc.tiling(256, 1000, 256, 10, True)[1:4] == (1, 32, 32)           # wide 256-thread tiles: base 32
    assert mc.tiling(256, 1000, 256, 12, True)[1:4] == (4, 8, 125)           # split: 64 columns, base 128
    t = mc.tiling(832, 160, 256, 14, False)                                   # want = ceil(160 * 13 / 256) = 9
    assert (t.nbx, t.ny, t.tchunk, t.n_tiles) == (13, 18, 9, 234) and t.lengths[-1] == 7
    assert mc.tiling(65, 5, 256, 14, False)[1:4] == (2, 1, 5)                # floor of 8 above H: one tile
    assert mc.tiling(262145, 2, 256, 12, False)[1:4] == (4097, 1, 2)         # the cap cannot cut nbx
    assert mc.tiling(8192, 8193, 256, 8, True)[1:4] == (32, 127, 65)         # the cap on ny: 4096 / 32 = 128 -> 65 steps


def _passes(split):
    return [(p, mc.tiling(p.R, p.H, p.block, p.D, p.riding)) for p in mc.gpu_passes()
            if mc.cov_split(p.D, p.block) == split]


@pytest.mark.parametrize("split", (False, True), ids=("wide", "split"))
def test_cases_reach_every_tile_length(split):
    lengths, ragged = set(), 0
    for p, t in _passes(split):
        lengths.update(t.lengths)
        ragged += t.ny > 1 and t.lengths[-1] < t.tchunk
    assert set(range(1, 14)) <= lengths, sorted(set(range(1, 14)) - lengths)
    assert ragged > 0


def test_cases_reach_every_tail_of_the_split_loop():
    """left = 1..4 as the whole tile; left = 2..4 behind at least one trip of the three-step loop.  left = 1 behind a
    trip does not exist: the loop runs while t + 4 < t1, so it leaves 2, 3 or 4 steps (checked here for every length)."""
    for length in range(5, 5000):
        trips, left = mc.split_tail(length)
        assert trips >= 1 and 2 <= left <= 4 and 3 * trips + left == length
    whole, behind = set(), set()
    for p, t in _passes(True):
        for length in t.lengths:
            trips, left = mc.split_tail(length)
            (behind if trips else whole).add(left)
    assert whole == {1, 2, 3, 4} and behind == {2, 3, 4}


@pytest.mark.parametrize("n", (3, 6))
def test_merge_cases_reach_every_tile_count(n):
    counts = [mc.tiling(R, H, mc.MOM_BLOCK, mc.dims(n), False).n_tiles for m, R, H in mc.MERGE_CASES if m == n]
    for k in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        assert k in counts, (n, k, sorted(counts))
    assert any(c > 320 for c in counts)
    for lo, hi in mc.N_TILES_CLASSES:
        assert any(lo <= c <= hi for c in counts)
    # and not only rows of column tiles: tile = by * nbx + bx with both above 1
    assert any(t.nbx > 1 and t.ny > 1 and t.n_tiles > 192
               for t in (mc.tiling(R, H, mc.MOM_BLOCK, mc.dims(n), False) for m, R, H in mc.MERGE_CASES if m == n))


def test_owed_cases_reach_the_fourth_partial_in_every_form():
    for (name, n), (n_dir, H) in mc.BIG_RIDING.items():
        f = [x for x in mc.RIDING_FORMS if (x.name, x.n) == (name, n)][0]
        t = mc.tiling(2 * n_dir, H, f.block, mc.dims(n), True)
        assert t.n_tiles > 192 and t.nbx > 1 and t.ny > 1, (name, n, t)
        assert 2 * n_dir * H * mc.dims(n) * 8 < 105e6
    assert {k[0] for k in mc.BIG_RIDING} == {"oct3", "quad3", "row", "lane"}
    assert {mc.cov_split(mc.dims(n), 256) for (name, n) in mc.BIG_RIDING if name == "row"} == {False, True}
    t = mc.tiling(*mc.CAP_CASE[1:], mc.MOM_BLOCK, mc.dims(mc.CAP_CASE[0]), False)
    assert t.nbx == 4097 and t.n_tiles == 4097


def test_cases_reach_the_edges_of_the_last_column_tile():
    """Live lanes of the last column tile: 1 and cols - 1 in the standalone pass, wide and split.  An owed pass has
    2 n_dir rollouts, so there it is 2 and cols - 2, at every tile width a form rides with."""
    live = {}
    for p in mc.gpu_passes():
        t = mc.tiling(p.R, p.H, p.block, p.D, p.riding)
        live.setdefault((p.where != "owed", p.block, t.cols), set()).add(p.R - (t.nbx - 1) * t.cols)
    assert {1, 255, 256} <= live[(True, 256, 256)] and {1, 63, 64} <= live[(True, 256, 64)]
    for block, cols in ((64, 64), (128, 128), (256, 256), (256, 64)):
        assert {2, cols - 2} <= live[(False, block, cols)], (block, cols, sorted(live[(False, block, cols)]))
    # every riding form has tiles along both axes, and a ragged last step tile
    for f in mc.RIDING_FORMS:
        ts = [mc.tiling(2 * nd, H, f.block, mc.dims(f.n), True) for nd, H in mc.riding_shapes(f)]
        assert any(t.ny > 1 and t.nbx > 1 for t in ts) and any(t.ny > 1 and t.lengths[-1] < t.tchunk for t in ts)
        assert any(t.ny == 3 for t in ts)


def test_every_owed_form_is_one_the_dispatch_has(sw):
    """The forms of RIDING_FORMS against the dispatch restated in tests/rollout_matrix_cases.py: each launch of the
    owed-pass tests (ARS, capture and V2 moments) reaches exactly one compiled rollout kernel of its form."""
    import rollout_matrix_cases as rc
    seen = set()
    for f in mc.RIDING_FORMS:
        form = "oct3" if f.name == "quad3" else f.name
        inst = rc.instantiation_of(form, f.n, True, True, True, f.flags, quad_env=f.quad_env)
        assert inst.form == f.name and inst.n == f.n
        seen.add(inst.symbol)
    assert len(seen) == len(mc.RIDING_FORMS)
    assert len({mc.riding_id(f) for f in mc.RIDING_FORMS}) == len(mc.RIDING_FORMS)


def test_the_exact_reference_is_the_long_double_one():
    for n, H, R in ((2, 7, 65), (3, 13, 300), (6, 9, 130), (8, 5, 66)):
        traj = mc.data("c", n, H, R)
        a, b = mc.reference_exact(traj), mc.reference(traj)
        assert a.count == b.count == H * R
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y)
        assert np.array_equal(mc.packed(a)[1:].astype(np.longdouble), np.concatenate((a.S1, a.S2.ravel())))
        # distinct enough: no two columns, steps or rollouts carry the same code
        k = mc.index_code(H, mc.dims(n), R)
        assert len({c.tobytes() for c in k.transpose(1, 0, 2)}) == mc.dims(n)
        assert len({c.tobytes() for c in k}) == H and len({c.tobytes() for c in k.transpose(2, 0, 1)}) == R


def test_the_regimes_are_what_they_claim():
    n, H, R = 5, 11, 130
    D = mc.dims(n)
    a = mc.centred(mc.data("a", n, H, R))
    assert (np.abs(a) >= 0.5 - 1e-15).all() and (np.abs(a) <= 2 + 1e-15).all()
    ra = mc.reference(mc.data("a", n, H, R))
    assert (np.abs(ra.S1) < 0.2 * ra.A1).all()                      # the sums cancel
    L = mc.additions(mc.tiling(R, H, 256, D, False), 256, D)
    assert float(mc.bounds(ra, L)[1].max()) < 1e-7 and float(mc.gamma(L)) * 4 * H * R < 0.25
    b = mc.data("b", n, H, R)
    assert (np.abs(b[:, :2]) > 999).all() and np.abs(mc.centred(b)[:, 2]).min() > 6 - 0.1
    rb = mc.reference(b)
    cov = rb.S2 / rb.count - np.outer(rb.S1, rb.S1) / rb.count ** 2
    assert (np.abs(np.diag(cov)) < 1e-6 * np.diag(rb.S2 / rb.count)[:2].max()).all()    # the host difference cancels


CASES_FOR_MUTANTS = ((3, 300, 9), (6, 100, 5), (4, 257, 13), (8, 65, 7))


@pytest.mark.parametrize("regime", ("a", "c"))
@pytest.mark.parametrize("kind", mc.MUTANTS)
def test_the_bound_shows_every_mutant(kind, regime):
    for n, R, H in CASES_FOR_MUTANTS:
        D = mc.dims(n)
        traj = mc.data(regime, n, H, R)
        ref = mc.reference(traj)
        t = mc.tiling(R, H, mc.MOM_BLOCK, D, False)
        L = mc.additions(t, mc.MOM_BLOCK, D)
        assert mc.violations(mc.packed(ref), ref, L) == []              # the reference itself passes
        bad = mc.violations(mc.mutate(kind, traj, ref, t, D), ref, L)
        assert bad, (kind, regime, n, R, H)
        if regime == "c":
            assert not np.array_equal(mc.mutate(kind, traj, ref, t, D), mc.packed(ref))


def test_the_bound_passes_float64_sums_in_the_kernels_order_and_counts_its_terms():
    """A float64 emulation of a wide tile pass in the kernel's order (lane sums, shuffle tree, wave partials, merge)
    stays inside the bound; L is the table of the module docstring."""
    assert mc.additions(mc.tiling(832, 160, 256, 14, False), 256, 14) == 9 + 6 + 0 + 1 + 2 + 6 + 1
    assert mc.additions(mc.tiling(65537, 1, 256, 8, False), 256, 8, earlier_passes=1) == 1 + 6 + 4 + 2 + 2 + 6 + 1 + 1
    n, R, H = 3, 300, 9
    D = mc.dims(n)
    traj = mc.data("a", n, H, R)
    x = mc.centred(traj)
    t = mc.tiling(R, H, 256, D, False)

    def shuffle(v):             # v [64, ...]: lane l += lane l + off, off = 32 .. 1
        v = v.copy()
        for off in (32, 16, 8, 4, 2, 1):
            v[:64 - off] = v[:64 - off] + v[off:]
        return v[0]
    rows = []
    for by in range(t.ny):
        for bx in range(t.nbx):
            lane = np.zeros((256, D + D * D))
            for step in range(by * t.tchunk, by * t.tchunk + t.lengths[by]):
                xs = np.zeros((256, D))
                live = min(256, R - bx * 256)
                xs[:live] = x[step, :, bx * 256:bx * 256 + live].T
                lane[:, :D] += xs
                lane[:, D:] += (xs[:, :, None] * xs[:, None, :]).reshape(256, D * D)    # (not fused: one more rounding)
            waves = [shuffle(lane[w * 64:(w + 1) * 64]) for w in range(4)]
            rows.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    part = np.zeros((64, 4, D + D * D))
    for i, row in enumerate(rows):
        part[i % 64, (i // 64) % 4] += row
    total = shuffle((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3]))
    got = np.concatenate(([float(H * R)], total))
    ref = mc.reference(traj)
    assert mc.violations(got, ref, mc.additions(t, 256, D) + 1) == []
    assert max(mc.ratios(got, ref)) > 0          # and it is not the reference itself
