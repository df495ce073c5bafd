"""The update matrix (tests/update_matrix_cases.py) without a GPU: that its kernel list IS what the library holds, that
its cases reach every path, that each case group would show the mistake it is there for, and that its references and
bounds are usable.

 * KERNEL LIST.  The kernel symbols of the built library whose own name is ars_update_kernel, ars_update_multi_kernel,
   ars_update_counted_kernel or ars_pack_admitted_kernel (names only, nothing read from the instructions) are exactly
   the seven of KERNELS; the launches of tests/test_update_matrix_gpu.py reach each of them, and within
   swimmer_update.inc every path: no selection, bitonic, LDS ranking, global ranking, deltas from registers and from
   global memory, the merge in one round and in more than one, at both workgroup sizes.
 * DISCRIMINATION.  A deliberately wrong restatement moves at least one compared value by more than 100 times its
   bound: ties to the lower index, ddof = 1 for sigma, the divisor b where the count is due and the reverse, the last
   moment row dropped, the rows of group G - 1 dropped, chunk = n_dir // world, agent a reading agent a + 1's slice,
   pack positions that restart at each wave or at each round.
 * CONDITIONING.  sigma of the used set >= 1e-3 of the returns' spread, M2 / n >= 1e-6, n1 - 1 > 0, and the rule
   recomputed in plain float64 with the sums taken in reversed order stays within the bound.
"""
import os
import re
import shutil

import numpy as np
import pytest

from test_loop_placement import LIB, LLVM, _disassemble

import update_matrix_cases as mc

needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and shutil.which(f"{LLVM}/llvm-objdump")),
                                 reason="needs the built library and the ROCm llvm tools")
FACTOR = 100.0


def _launched():
    """The kernels that the launches of the GPU test reach."""
    out = set()
    for n in mc.NS:
        out |= {("ars_update_kernel", mc.block_of(n_dir)) for n_dir in mc.n_dirs(n)}
        out |= {("ars_update_multi_kernel", mc.block_of(n_dir)) for n_dir in mc.MULTI_N_DIRS}
    out.add(("ars_update_counted_kernel", mc.BLOCK))
    if mc.COUNTED_MAX >= mc.WIDE_FROM:
        out.add(("ars_update_counted_kernel", mc.BLOCK_WIDE))
    out.add(("ars_pack_admitted_kernel", None))
    return out


def test_the_list_has_seven_kernels_and_the_gpu_test_launches_each():
    assert len(mc.KERNELS) == 7 and len({mc.symbol(*k) for k in mc.KERNELS}) == 7
    assert _launched() == set(mc.KERNELS)
    # the counted launch runs both sizes, and both serve an agent: counts on either side of the switch
    sizes = {mc.block_of(mc.counted_n_dir(c)) for c in mc.COUNTS if mc.counted_n_dir(c) > 0}
    assert sizes == {mc.BLOCK, mc.BLOCK_WIDE}
    assert {mc.counted_n_dir(c) for c in mc.COUNTS} >= {0, mc.WIDE_FROM - 1, mc.WIDE_FROM, mc.COUNTED_MAX}


@needs_tools
def test_every_compiled_kernel_of_the_family_is_listed_once():
    pattern = re.compile("(?:" + "|".join(f"{len(k)}{k}[IE]" for k in mc.KERNEL_NAMES) + ")")
    symbols = sorted({l.split("<", 1)[1][:-2] for l in _disassemble()
                      if l.startswith("0000") and l.endswith(">:") and pattern.search(l)})
    assert len(symbols) == 7, symbols
    for s in symbols:
        assert sum(mc.symbol(*k) in s for k in mc.KERNELS) == 1, s
    for k in mc.KERNELS:
        assert sum(mc.symbol(*k) in s for s in symbols) == 1, (k, "is not in the library")


def test_every_path_has_cases():
    small, wide = mc.BLOCK, mc.BLOCK_WIDE
    every = {(small, "none", "registers"), (small, "bitonic", "registers"), (wide, "none", "registers"),
             (wide, "bitonic", "registers"), (wide, "lds_rank", "registers"), (wide, "none", "global"),
             (wide, "global_rank", "global")}
    for n in (2, 8):                                             # the extremes of md run the whole list
        assert {mc.path(n_dir, tb) for n_dir in mc.n_dirs(n) for tb in mc.top_bs(n_dir)} == every
    for n in mc.NS:
        got = {mc.path(n_dir, tb) for n_dir in mc.n_dirs(n) for tb in mc.top_bs(n_dir)}
        assert got >= {p for p in every if p[2] == "registers"}, n
        assert set(mc.n_dirs(n)) >= set(mc.N_DIRS_EVERY)
        merges = {mc.merge_path(n, n_dir, rows) for n_dir in (5, 1025)
                  for rows in mc.moment_rows(n, mc.block_of(n_dir))}
        assert merges == {(b, r) for b in (small, wide) for r in ("one_round", "more_rounds")}, n
        for block in (small, wide):
            G = mc.groups(n, block)
            assert set(mc.moment_rows(n, block)) == {1, G - 1, G, G + 1, 8 * G, 8 * G + 1}
    # the sizes at which the code takes another path are in the list, on both sides
    for edge in (mc.WAVE, mc.BLOCK, mc.WIDE_FROM - 1, mc.SORT_DIRS, mc.LDS_DIRS):
        assert {edge, edge + 1} <= set(mc.N_DIRS_FULL)
    assert all(len(mc.top_bs(n_dir)) == len(set(mc.top_bs(n_dir))) for n_dir in mc.N_DIRS_FULL)
    assert mc.top_bs(700) == (0, 1, 233, 699, 700, 707) and mc.top_bs(1) == (0, 1, 8)


def _moved(wrong, ref):
    """The largest |wrong - reference| / bound over the compared values of a result ({name: Ref})."""
    return max(mc.ratio(np.asarray(wrong[k].value, dtype=np.float64), ref[k]) for k in ref)


def _update(inp, top_b, **wrong):
    return mc.reference_update(inp["returns"], inp["deltas"], inp["policy"], inp["alpha"], inp["b"], top_b, **wrong)


@pytest.mark.parametrize("n", mc.NS)
def test_the_update_cases_discriminate_and_are_well_conditioned(n):
    worst = 0.0
    for n_dir in mc.n_dirs(n):
        inp = mc.inputs(n, n_dir)
        ret = inp["returns"]
        assert np.isfinite(ret).all() and inp["b"] != n_dir
        keys = np.maximum(ret[0::2], ret[1::2])
        assert n_dir < 6 or len(np.unique(keys)) <= n_dir // 3          # many exact ties
        spread = ret.max() - ret.min()
        ties = []
        for top_b in mc.top_bs(n_dir):
            ref = _update(inp, top_b)
            assert np.isfinite(ref["policy"].value.astype(np.float64)).all()
            assert float(ref["sigma"].value) >= 1e-3 * spread, (n_dir, top_b)
            assert _moved(_update(inp, top_b, ddof=1), ref) > FACTOR, (n_dir, top_b, "ddof")
            assert _moved(_update(inp, top_b, divisor="swapped"), ref) > FACTOR, (n_dir, top_b, "divisor")
            if 0 < top_b < n_dir:
                ties.append(_moved(_update(inp, top_b, ties="lower"), ref))
            # the bound holds for the rule itself in plain float64, every sum from its last term to its first
            pol, sigma = mc.float64_update(ret, inp["deltas"], inp["policy"], inp["alpha"], inp["b"], top_b)
            r = max(mc.ratio(pol, ref["policy"]), mc.ratio(sigma, ref["sigma"]))
            worst = max(worst, r)
            assert r <= 1.0, (n_dir, top_b, r)
        if n_dir >= 2:                                             # every boundary that selects sits inside a tie
            assert ties and min(ties) > FACTOR, (n_dir, ties)
    print(f"n = {n}: plain float64 in reversed order is within {worst:.3f} of the bound")


def _drop_last(u, rows):
    return rows[:-1]


@pytest.mark.parametrize("n", mc.NS)
def test_the_moment_cases_discriminate_and_are_well_conditioned(n):
    names = ("running", "mean", "inv_std")
    for n_dir in (5, 1025):
        block = mc.block_of(n_dir)
        G = mc.groups(n, block)
        assert (block - G * 2 * mc.dims(n)[0] > 0) == (n not in (3, 7))   # idle threads unless 2d is a power of two
        for rows in mc.moment_rows(n, block):
            batches, refs = mc.moment_case(n, n_dir, rows)
            assert [b["rows"].shape for b in batches] == [(rows, 2 * mc.dims(n)[0])] * 3
            news = [b["n_new"] for b in batches]
            assert news[0] != news[1] and min(news) > 1
            # the batch means move apart by far more than the bound: the delta term of the merge matters
            means = [b["rows"][:, :mc.dims(n)[0]].sum(axis=0) / b["n_new"] for b in batches]
            assert np.abs(means[1] - means[0]).max() > 0.3 and np.abs(means[2] - means[1]).max() > 0.3
            assert np.abs(means[1] - means[0]).min() > 1e-6 and np.abs(means[2] - means[1]).min() > 1e-6
            n1 = 0
            for u, ref in enumerate(refs):
                n1 += news[u]
                run = ref["running"].value.astype(np.float64)
                assert run[0] == n1 and n1 - 1 > 0
                assert (run[1 + mc.dims(n)[0]:] / n1 >= 1e-6).all()
                assert np.isfinite(ref["inv_std"].value.astype(np.float64)).all()
            # the merge restated from the rows agrees with the list of states; so does plain float64 backwards
            for got in (mc.merge_from_rows(n, batches), mc.merge_from_rows(n, batches, reverse=True, dtype=np.float64)):
                for u, ref in enumerate(refs):
                    for k, g in zip(names, got[u]):
                        assert mc.ratio(g.astype(np.float64), ref[k]) <= 1.0, (n_dir, rows, u, k)
            wrongs = [("last row", _drop_last)]
            if rows >= G:
                wrongs.append(("group G - 1", lambda u, r: r[np.arange(len(r)) % G != G - 1]))
            for what, drop in wrongs:
                with np.errstate(all="ignore"):
                    bad = mc.merge_from_rows(n, batches, drop=drop)
                for u, ref in enumerate(refs):
                    moved = max(mc.ratio(g.astype(np.float64), ref[k]) for k, g in zip(names, bad[u]))
                    assert moved > FACTOR, (n_dir, rows, u, what, moved)


@pytest.mark.parametrize("n", mc.GATHERED_NS)
def test_the_gathered_cases_discriminate(n):
    d = mc.dims(n)[0]
    for n_dir in mc.GATHERED_N_DIRS + mc.GATHERED_ALIGNED:
        inp = mc.inputs(n, n_dir)
        top_b = n_dir // 3
        ref = _update(inp, top_b)
        for world in mc.GATHERED_WORLDS:
            c = mc.gathered_case(n, n_dir, world)
            chunk, rows_chunk = c["chunk"], c["rows_chunk"]
            assert chunk == -(-n_dir // world) and world * chunk >= n_dir
            assert mc.row_aligned(n_dir, world) == (n_dir in mc.GATHERED_ALIGNED)
            assert (n_dir in mc.GATHERED_ALIGNED) or world == 1 or world * chunk > n_dir        # a ragged last chunk
            for u, buf in enumerate(c["buffers"]):
                assert buf.shape == (world * (2 * chunk + rows_chunk * 2 * d),)
                assert np.array_equal(mc.gathered_returns(buf, n, n_dir, world, chunk, rows_chunk), inp["returns"])
                seg = buf.reshape(world, -1)
                slots = seg[:, :2 * chunk].ravel()
                assert (slots[2 * n_dir:] == mc.POISON).all() if world * chunk > n_dir else True
                # the segments' rows, padding included, add up to the batch's rows
                got = seg[:, 2 * chunk:].reshape(world * rows_chunk, 2 * d)
                real = got[np.abs(got).sum(axis=1) > 0]
                assert np.array_equal(real, c["batches"][u]["rows"])
                if mc.row_aligned(n_dir, world):
                    assert np.array_equal(got, mc.gathered_case(n, n_dir, 1)["batches"][u]["rows"])
            floor = n_dir // world
            if world > 1 and floor >= 1 and floor != chunk:
                bad = mc.gathered_returns(c["buffers"][0], n, n_dir, world, chunk, rows_chunk, index_chunk=floor)
                try:
                    wrong = mc.reference_update(bad, inp["deltas"], inp["policy"], inp["alpha"], inp["b"], top_b)
                    moved = _moved(wrong, ref)
                except ZeroDivisionError:      # the one used direction is a poisoned slot: sigma = 0, an infinite step
                    moved = np.inf
                assert moved > FACTOR, (n_dir, world)
            else:      # nothing to get wrong: one rank, shards that divide, or fewer directions than ranks
                assert world == 1 or n_dir % world == 0 or n_dir < world


@pytest.mark.parametrize("n", mc.NS)
def test_the_agents_of_a_multi_case_are_unrelated(n):
    for n_dir in mc.MULTI_N_DIRS:
        c = mc.multi_case(n, n_dir)
        S = mc.MULTI_AGENTS
        refs = [_update(a, c["top_b"]) for a in c["agents"]]
        assert 0 < c["top_b"] < n_dir and all(b[0]["rows"].shape[0] == mc.rows_of(n_dir) for b in c["batches"])
        for a in range(S):
            nxt = (a + 1) % S
            for k in ("policy", "sigma"):          # every compared value on its own: one shared buffer would show
                assert mc.ratio(refs[nxt][k].value.astype(np.float64), refs[a][k]) > FACTOR, (n_dir, a, k)
            for u in range(2):
                for k in ("running", "mean", "inv_std"):
                    other = c["refs_v2"][nxt][u][k].value.astype(np.float64)
                    assert mc.ratio(other, c["refs_v2"][a][u][k]) > FACTOR, (n_dir, a, u, k)


@pytest.mark.parametrize("n", mc.COUNTED_NS)
def test_the_agents_of_the_counted_case_are_unrelated(n):
    c = mc.counted_case(n)
    S, N = len(mc.COUNTS), mc.COUNTED_MAX
    d, m, _ = mc.dims(n)
    assert c["returns"].shape == (S, 2 * N) and c["deltas"].shape == (S, N, m, d)
    assert c["moments"].shape == (S, mc.rows_of(N), 2 * d) and c["running"].shape == (S, 1 + 2 * d)
    assert (c["running"][:, 0] > 0).all() and (c["running"][:, 1 + d:] > 0).all()
    for a in range(S):
        nxt = (a + 1) % S
        for count in (5, N):
            for top_b in mc.COUNTED_TOP_B:
                tb = min(top_b, count)
                own = mc.reference_update(c["returns"][a, :2 * count], c["deltas"][a, :count], c["policy"][a],
                                          c["alpha"], c["b"], tb)
                other = mc.reference_update(c["returns"][nxt, :2 * count], c["deltas"][nxt, :count], c["policy"][a],
                                            c["alpha"], c["b"], tb)
                assert mc.ratio(other["sigma"].value.astype(np.float64), own["sigma"]) > FACTOR
                assert mc.ratio(other["policy"].value.astype(np.float64), own["policy"]) > FACTOR
        assert np.abs(c["moments"][a] - c["moments"][nxt]).min() > 1e-6


@pytest.mark.parametrize("n_dir", mc.PACK_N_DIRS)
def test_the_pack_cases_discriminate(n_dir):
    for n in mc.PACK_NS:
        shown = {mc.WAVE: [], mc.PACK_BLOCK: []}
        for name in mc.PACK_PATTERNS:
            for with_status in (False, True):
                c = mc.pack_case(n, n_dir, name, with_status)
                count, order, packed = mc.reference_pack(c["admit"], c["status"], c["deltas"])
                on = c["admit"] != 0
                if with_status:
                    refused = (c["status"][:, 0::2] != 0) | (c["status"][:, 1::2] != 0)
                    assert refused.any()
                    on &= ~refused
                for a in range(mc.PACK_AGENTS):
                    assert count[a] == on[a].sum()
                    assert np.array_equal(order[a, :count[a]], np.flatnonzero(on[a]))
                    assert (order[a, count[a]:] == -1).all()
                    assert np.array_equal(packed[a, :count[a]], c["deltas"][a][on[a]])
                    assert np.isnan(packed[a, count[a]:]).all()
                for restart in shown:
                    bad = mc.reference_pack(c["admit"], c["status"], c["deltas"], restart=restart)
                    shown[restart].append((name, not np.array_equal(bad[1], order)))
        # positions that restart at each wave show as soon as there is a second wave, at each round with a second round
        for restart, seen in shown.items():
            if n_dir > restart:
                assert any(s for _, s in seen), (n_dir, restart)
                assert seen[0] == ("all", True), (n_dir, restart, seen)          # every direction, no status
            else:
                assert not any(s for _, s in seen)
