"""get_opt_hclust_batch, the driver that every base clustering, wMetaC and sMetaC goes through, tested DIRECTLY: short lists of tiny
tasks through sharp_get_opt_hclust_batch (one driver call), one list per regime of the driver -- agglomeration form, ranges, chunks and
buffer sets, deferred fallback, chunk-wide statistics switches, running buffer offsets of mixed tasks, nested batches.

Every test first asserts the PLAN the driver recorded (sharp_hclust_batch_plan: chunks, slots, split / 1024 / 512 form, NS, ml,
deferred fallback), so that a changed heuristic cannot quietly turn a regime test into a copy of another, and then checks EVERY task:
  (a) against the oracle (tests/_hclust_batch_ref.py; one task at a time), with the project's tolerances: height rtol 1e-9 atol 1e-12,
      msil atol 1e-10, CHind rtol 1e-8 where finite, f, v, optN, branch equal;
  (b) against the same task run ALONE through sharp_get_opt_hclust: f, v, branch equal, height rtol 1e-12 atol 1e-14 (the bound between
      agglomeration forms), msil atol 1e-12 and CHind rtol 1e-10 (the bounds between statistics kernels);
  (c) `sequential` as planned: 1 exactly for tasks with exact ties and for centroid / median;
  (d) no sentinel left in any output;
  (e) a second identical call returns identical bits (the workspaces are reused).
No task is skipped: every task of every list passes _hclust_batch_ref.check_margins (asserted on the CPU and again here)."""
import numpy as np
import pytest

import _hclust_batch_ref as ref
from sharp_amd import hclust_batch as hb

pytestmark = pytest.mark.gpu

FLOATS = ("height", "msil", "CHind")
INTS = ("f", "v")
SCALARS = ("optN", "nk", "branch", "rc", "sequential")


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def num_cu(sa):
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _tasks(name):
    """a list, its oracle results, and the proof that every task of it can be compared exactly (never a skip)"""
    tasks, refs = ref.reference(name)
    assert ref.margin_failures(name) == []
    return tasks, refs


def _batch(tasks, nested=False):
    res = hb.get_opt_hclust_batch(list(tasks), want_v=True, nested=nested)
    return res, hb.batch_plan()


_ALONE = {}


def _alone(sa, tasks):
    """every task on its own through sharp_get_opt_hclust, with the library's defaults (call it before any switch is set); once per
    distinct task"""
    out = []
    for t in tasks:
        key = (id(t["mat"]), t["kind"], t["hmethod"], t["N_cluster"], t["minN"], t["maxN"], t["sil_thre"], t["height_Ntimes"])
        if key not in _ALONE:
            _ALONE[key] = (t["mat"], sa.get_opt_hclust(t["mat"], hmethod=t["hmethod"], N_cluster=t["N_cluster"] or None,
                                                       minN_cluster=t["minN"], maxN_cluster=t["maxN"], sil_thre=t["sil_thre"],
                                                       height_Ntimes=t["height_Ntimes"]))
        out.append(_ALONE[key][1])
    return out


def _assert_plan(plan, expect):
    """`expect`: one dict per chunk with the columns that the test pins"""
    assert len(plan) == len(expect), plan
    for row, want in zip(plan, expect):
        assert {k: row[k] for k in want} == want, (row, plan)


def _same_bits(a, b):
    for x, y in zip(a, b):
        for key in FLOATS:
            assert np.array_equal(x[key].view(np.uint64), y[key].view(np.uint64)), key
        for key in INTS:
            assert np.array_equal(x[key], y[key]), key
        for key in SCALARS:
            assert x[key] == y[key], key


def _no_sentinel(r):
    for key in FLOATS + INTS:
        assert not hb.is_sentinel(r[key]).any(), key
    for key in SCALARS:
        assert r[key] != hb.INT_SENTINEL, key


def _vs_oracle(task, r, want):
    np.testing.assert_allclose(r["height"], want["height"], rtol=1e-9, atol=1e-12)
    assert r["rc"] == want["rc"] and r["nk"] == want["msil"].size
    if task.get("saturated"):       # as test_get_opt_hclust_symmetric_similarity: the arg-max pattern of msil (exact ties) and f
        assert np.array_equal(r["msil"] == r["msil"].max(), want["msil"] == want["msil"].max())
        assert np.array_equal(r["f"], want["f"]) and r["optN"] == want["optN"] and r["branch"] == want["branch"]
        return
    np.testing.assert_allclose(r["msil"], want["msil"], rtol=0, atol=1e-10)
    if task["N_cluster"] > 0:
        assert np.isnan(r["CHind"][0])          # the batch leaves it: the Euclidean index is the single-task wrapper's
    else:
        fin = np.isfinite(want["CHind"])
        np.testing.assert_allclose(r["CHind"][fin], want["CHind"][fin], rtol=1e-8)
    assert r["optN"] == want["optN"] and r["branch"] == want["branch"]
    assert np.array_equal(r["f"], want["f"]) and np.array_equal(r["v"], want["v"])


def _vs_alone(task, r, one):
    assert np.array_equal(r["f"], one["f"]) and np.array_equal(r["v"], one["v"]) and r["branch"] == one["branch"]
    np.testing.assert_allclose(r["height"], one["height"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["msil"], one["msil"], rtol=0, atol=1e-12)
    if task["N_cluster"] == 0:
        fin = np.isfinite(one["CHind"])
        assert np.array_equal(fin, np.isfinite(r["CHind"]))
        np.testing.assert_allclose(r["CHind"][fin], one["CHind"][fin], rtol=1e-10)


def _run(tasks, refs, alone, expect_plan, sequential=None, exact=FLOATS):
    """one batch: plan, then (a) - (e) for every task; returns the results.  exact: the outputs that equal the task's run alone BIT FOR
    BIT, beyond the bounds of (b) -- measured on the MI355X: every form of the bulk-synchronous agglomeration merges in the same order
    with the same arithmetic (round per launch with any geometry, one launch of 1024 or 512 threads, state in LDS or global memory), a
    task's distance matrix and statistics do not depend on its neighbours in the chunk, its range or its buffer set; so everything is
    exact unless the chunk takes another statistics kernel than the task alone (the callers say so) or the sequential kernel is forced."""
    res, plan = _batch(tasks)
    _assert_plan(plan, expect_plan)
    again, plan2 = _batch(tasks)
    assert plan2 == plan
    _same_bits(res, again)                                                        # (e)
    assert len(res) == len(tasks)
    for i, (t, r, want, one) in enumerate(zip(tasks, res, refs, alone)):
        try:
            _no_sentinel(r)                                                       # (d)
            _vs_oracle(t, r, want)                                                # (a)
            _vs_alone(t, r, one)                                                  # (b)
            for key in exact:
                if key != "CHind" or t["N_cluster"] == 0:
                    assert np.array_equal(r[key].view(np.uint64), one[key].view(np.uint64)), f"{key} differs in bits from the task alone"
            assert r["sequential"] == (ref.expected_sequential(t) if sequential is None else sequential)   # (c)
        except AssertionError as e:
            raise AssertionError(f"task {i} (n = {t['mat'].shape[0]}, kind {t['kind']}, {t['hmethod']}): {e}") from e
    return res


ONE_CHUNK = dict(slot=0, pipe=0, nested=0, seq_deferred=0)


def test_mixed_sizes_in_the_round_per_launch_form(sa, num_cu, monkeypatch):
    """One task of 1000 observations puts the whole chunk on the round-per-launch agglomeration; the tasks of 3 .. 300 observations finish
    within the first rounds (the `remaining` counter, the host's look every eighth round, the empty workgroups of finished tasks).  The
    same list with MODE 3 at round 3 and never, 1 and 5 workgroups per task, and in one 1024-thread launch (SHARP_HC_SPLIT=0,
    SHARP_HC_MONO=1): every run against the same oracle results, and within the bound between agglomeration forms of the task alone."""
    tasks, refs = _tasks("mixed_sizes")
    alone = _alone(sa, tasks)
    n = len(tasks)
    split = dict(ONE_CHUNK, i0=0, i1=n, split=1, form=hb.FORM_SPLIT, NS=1, ml=0, gs=0, max_n=1000, max_kpad=16, finish_at=15)
    base = _run(tasks, refs, alone, [dict(split, wpt=8) if num_cu == ref.NUM_CU else split])
    assert hb.batch_plan()[0]["wpt"] not in (1, 5)
    # the plan reports the geometry that RAN (a switch that the library did not read would leave finish_at = 15 and the default wpt)
    for name, value, ran in [("SHARP_HC_FINISH_AT", "3", dict(finish_at=3)), ("SHARP_HC_FINISH_AT", "-1", dict(finish_at=-1)),
                             ("SHARP_HC_WPT", "1", dict(wpt=1)), ("SHARP_HC_WPT", "5", dict(wpt=5))]:
        monkeypatch.setenv(name, value)
        res = _run(tasks, refs, alone, [dict(split, **ran)])
        monkeypatch.delenv(name)
        for a, b in zip(res, base):                 # the same merges whatever the launch geometry
            assert np.array_equal(a["v"], b["v"])
    monkeypatch.setenv("SHARP_HC_SPLIT", "0")
    _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=n, split=0, form=hb.FORM_1024, NS=1, gs=0, wpt=0, finish_at=0)])
    monkeypatch.delenv("SHARP_HC_SPLIT")
    monkeypatch.setenv("SHARP_HC_MONO", "1")
    _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=n, split=1, form=hb.FORM_1024, NS=1, gs=0, wpt=0, finish_at=0)])


def test_every_linkage_in_one_batch(sa):
    """The method is read per task (HcMeta::method): six reducible linkages by the bulk-synchronous kernel, centroid and median by the
    sequential one, in one chunk."""
    tasks, refs = _tasks("linkages")
    res = _run(tasks, refs, _alone(sa, tasks), [dict(ONE_CHUNK, i0=0, i1=8, split=0, form=hb.FORM_1024, NS=1, ml=0, gs=0)])
    assert [r["sequential"] for r in res] == [0] * 6 + [1, 1]


def test_feature_and_similarity_tasks_interleaved(sa):
    """F, S, S, F, S and a saturated S: D0 advances for similarity tasks only, the T^T = H^T D0 GEMM list is shorter than the others,
    row preparation without the all-feature-rows shortcut.  The last task (wMetaC of identical partitions, exact ones off the diagonal)
    is checked as test_get_opt_hclust_symmetric_similarity checks it; its exact ties send it to the sequential kernel."""
    tasks, refs = _tasks("interleaved")
    assert [t["kind"] for t in tasks] == [0, 1, 1, 0, 1, 1]
    _run(tasks, refs, _alone(sa, tasks), [dict(ONE_CHUNK, i0=0, i1=6, split=0, form=hb.FORM_1024, NS=1, ml=0, max_n=200, max_kpad=32)])


def test_row_minimum_parts_for_some_tasks_only(sa, monkeypatch):
    """n = 2049 (nld 2176: no parts), 300, a similarity task, 2048: the row-minimum buffer advances for the second and fourth task only.
    With SHARP_HC_NN_GEMM=0 (the first round scans D) the results are bit-equal, as the single-task test demands."""
    tasks, refs = _tasks("nn_parts")
    alone = _alone(sa, tasks)
    plan = [dict(ONE_CHUNK, i0=0, i1=4, split=1, form=hb.FORM_SPLIT, NS=1, gs=0, max_n=2049)]
    a = _run(tasks, refs, alone, plan)
    monkeypatch.setenv("SHARP_HC_NN_GEMM", "0")
    b = _run(tasks, refs, alone, plan)
    _same_bits(a, b)


def test_one_task_with_70_finest_clusters_moves_the_chunk_to_stats_kernel(sa):
    """maxN 15, 16, 17, 40, 64: kpad differs per task and the chunk takes stats_lane_kernel (max_kpad 64); with a sixth task of maxN = 70
    the whole chunk takes stats_kernel (max_kpad 80).  The two kernels add in the same order per cell: msil of the common tasks equal."""
    tasks, refs = _tasks("kpad")
    alone = _alone(sa, tasks)
    with70 = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=6, NS=1, ml=0, max_kpad=80, form=hb.FORM_1024)],
                  exact=("height", "msil"))    # (CH: stats_kernel associates a cluster's Gram sums otherwise than the lane kernel of the task alone)
    without = _run(tasks[:5], refs[:5], alone[:5], [dict(ONE_CHUNK, i0=0, i1=5, NS=1, ml=0, max_kpad=64, form=hb.FORM_1024)])
    for a, b in zip(with70, without):
        assert np.array_equal(a["msil"], b["msil"]) and np.array_equal(a["v"], b["v"])
        np.testing.assert_allclose(a["CHind"], b["CHind"], rtol=1e-12)
        assert np.array_equal(a["height"], b["height"])


def test_many_levels_statistics_are_chunk_wide(sa, monkeypatch):
    """SHARP_ML_MIN_LEVELS=8: one task with 30 candidate levels sends the tasks with 3 levels and with 1 (N_cluster given), a similarity
    task among them, through ml_*_kernel too.  Against the per-level kernels (SHARP_ML_MIN_LEVELS=100000) within the bounds between the
    statistics kernels."""
    tasks, refs = _tasks("many_levels")
    alone = _alone(sa, tasks)
    monkeypatch.setenv("SHARP_ML_MIN_LEVELS", "8")
    a = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=4, NS=1, ml=1, max_nk=30)], exact=("height",))
    monkeypatch.setenv("SHARP_ML_MIN_LEVELS", "100000")
    b = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=4, NS=1, ml=0, max_nk=30)])
    for t, x, y in zip(tasks, a, b):
        np.testing.assert_allclose(x["msil"], y["msil"], rtol=0, atol=1e-12)
        if t["N_cluster"] == 0:
            np.testing.assert_allclose(x["CHind"], y["CHind"], rtol=1e-10)
        assert np.array_equal(x["v"], y["v"]) and np.array_equal(x["height"], y["height"])


def test_given_cluster_numbers_beside_ranges_and_a_short_task(sa):
    """N_cluster given (one level, CHind left NaN) beside ranged tasks, features and similarity, a task with n - 1 < maxN (n = 12,
    maxN = 40: ten levels, the last all but one singleton), and two weakly structured tasks whose level the CH rule and the height rule
    choose."""
    tasks, refs = _tasks("given_and_short")
    assert [r["branch"] for r in refs] == [0, 0, 0, 0, 0, 1, 2]
    res = _run(tasks, refs, _alone(sa, tasks), [dict(ONE_CHUNK, i0=0, i1=7, NS=1, ml=0, max_kpad=48, max_nk=39, form=hb.FORM_1024)])
    assert [r["nk"] for r in res] == [1, 39, 10, 1, 7, 39, 39] and res[0]["optN"] == 3 and res[3]["optN"] == 4
    assert [r["branch"] for r in res] == [0, 0, 0, 0, 0, 1, 2]


def test_fallback_inside_a_batch(sa, monkeypatch):
    """Five tasks of about 300 observations, tasks 1 and 3 with duplicated rows.  One chunk: the sequential fallback is launched at once.
    SHARP_HC_CHUNK=2: three pipelined chunks on three buffer sets, both tie tasks in chunks with a successor (fallback deferred to the
    statistics phase).  SHARP_HC_CHUNK=3: two pipelined chunks on two sets, a tie task in the first (deferred) and one in the last
    (launched at once).  SHARP_HC_PIPE=0: chunk after chunk.  SHARP_HC_SEQ=1: the sequential kernel only.  Same results in all."""
    tasks, refs = _tasks("fallback")
    alone = _alone(sa, tasks)
    # the pipelined runs first: the merge lists that the buffers still hold are then another test's, and a fallback that never ran shows
    monkeypatch.setenv("SHARP_HC_CHUNK", "2")
    piped = dict(pipe=1, NS=1, split=0, form=hb.FORM_1024, nested=0)
    three = _run(tasks, refs, alone, [dict(piped, i0=0, i1=2, slot=0, seq_deferred=1), dict(piped, i0=2, i1=4, slot=1, seq_deferred=1),
                                      dict(piped, i0=4, i1=5, slot=3, seq_deferred=0)])
    monkeypatch.setenv("SHARP_HC_CHUNK", "3")
    two = _run(tasks, refs, alone, [dict(piped, i0=0, i1=3, slot=0, seq_deferred=1), dict(piped, i0=3, i1=5, slot=1, seq_deferred=0)])
    monkeypatch.setenv("SHARP_HC_CHUNK", "2")
    monkeypatch.setenv("SHARP_HC_PIPE", "0")
    serial = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=i0, i1=i1, NS=1, form=hb.FORM_1024) for i0, i1 in [(0, 2), (2, 4), (4, 5)]])
    monkeypatch.delenv("SHARP_HC_PIPE")
    monkeypatch.delenv("SHARP_HC_CHUNK")
    base = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=5, NS=1, split=0, form=hb.FORM_1024)])
    assert [r["sequential"] for r in base] == [0, 1, 0, 1, 0]
    monkeypatch.setenv("SHARP_HC_SEQ", "1")
    seq = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=5, NS=1, form=hb.FORM_NONE)], sequential=1, exact=("msil", "CHind"))
    for other in (three, two, serial):              # the same kernels on the same task, whatever the chunking: the same bits
        _same_bits(base, other)
    for a, b in zip(seq, base):
        assert np.array_equal(a["v"], b["v"]) and np.array_equal(a["f"], b["f"]) and a["branch"] == b["branch"]


def test_two_ranges_and_three(sa, monkeypatch):
    """194 ragged tasks: one chunk in two ranges of 97 on two streams; tie tasks at 0, 96, 97 and 193 sit on both sides of the range
    boundary, and one at 150 has a task without ties at its place in the other range (status + R.t0).  Then seven tasks with SHARP_HC_RANGES=3: uneven ranges [0, 2), [2, 4), [4, 7), a tie task in the middle."""
    tasks, refs = _tasks("two_ranges")
    res = _run(tasks, refs, _alone(sa, tasks), [dict(ONE_CHUNK, i0=0, i1=194, NS=2, split=0, form=hb.FORM_1024, ml=0)])
    assert [i for i, r in enumerate(res) if r["sequential"]] == [0, 96, 97, 150, 193]
    tasks, refs = _tasks("three_ranges")
    alone = _alone(sa, tasks)
    monkeypatch.setenv("SHARP_HC_RANGES", "3")
    res = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=7, NS=3, split=0, form=hb.FORM_1024)])
    assert [r["sequential"] for r in res] == [0, 0, 0, 1, 0, 0, 0]


def _expected_bounds(count, ncu):
    """A TRANSCRIPTION of the driver's chunk rule (it only carries the test to devices with another number of CUs; the check proper is
    the literal bounds for 256 CUs in the test).  The rule in the comments of get_opt_hclust_batch: more tasks than CUs -> equal chunks of at most one task per CU, from three
    chunks on of at most 3/4 of the CUs; with more than two chunks' worth of tasks a first chunk of max(140, 4/5 of a chunk) and the rest
    in equal chunks again"""
    per = count
    if count > ncu:
        nch = -(-count // ncu)
        if nch >= 3:
            nch = -(-count // (ncu * 3 // 4))
        per = -(-count // nch)
    first = 0
    if count > 2 * per:
        want = max(ref.K_SPLIT_MAX_TASKS + 4, per * 4 // 5)
        if want < per:
            first = want
            rest = count - first
            per = -(-rest // -(-rest // per))
    bounds, i0 = [], 0
    while i0 < count:
        i1 = min(count, i0 + (first if i0 == 0 and first else per))
        bounds.append((i0, i1))
        i0 = i1
    return bounds


def test_more_tasks_than_compute_units(sa, num_cu, monkeypatch):
    """257 tasks: two pipelined chunks (129 + 128 on a 256-CU device) on sets 0 and 1.  513: a first chunk of 140, then equal chunks, three
    sets in rotation (0, 1, 3, 0).  300 tasks with SHARP_HC_CHUNK=300: one chunk -- of two ranges of 150, each a 1024-thread launch; with
    SHARP_HC_RANGES=1 as well it is one range of 300 > CUs: the 512-thread form.  A handful of tie tasks spread over the chunks."""
    slots = [0, 1, 3]
    for count in (257, 513):
        tasks, refs = _tasks(f"many_{count}")
        bounds = _expected_bounds(count, num_cu)
        if num_cu == ref.NUM_CU:      # (an MI355X: the bounds written out, not computed)
            assert bounds == {257: [(0, 129), (129, 257)], 513: [(0, 140), (140, 265), (265, 390), (390, 513)]}[count]
        R = 3 if len(bounds) >= 3 else 2
        plan = [dict(i0=b[0], i1=b[1], slot=slots[j % R], pipe=1, NS=1, split=0, form=hb.FORM_1024, nested=0, ml=0,
                     seq_deferred=int(j + 1 < len(bounds))) for j, b in enumerate(bounds)]
        res = _run(tasks, refs, _alone(sa, tasks), plan)
        assert [i for i, r in enumerate(res) if r["sequential"]] == [i for i, t in enumerate(tasks) if t["tie"]]
    tasks, refs = _tasks("many_300")
    alone = _alone(sa, tasks)
    monkeypatch.setenv("SHARP_HC_CHUNK", "300")
    a = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=300, NS=2, split=0, form=hb.FORM_1024)])
    if num_cu < 300:
        monkeypatch.setenv("SHARP_HC_RANGES", "1")
        b = _run(tasks, refs, alone, [dict(ONE_CHUNK, i0=0, i1=300, NS=1, split=0, form=hb.FORM_512)])
        for x, y in zip(a, b):
            assert np.array_equal(x["v"], y["v"])


def test_state_in_global_memory_for_a_whole_chunk(sa):
    """n = 4100, 50, 1000: one task beyond 4096 observations makes every task of the chunk run the kernels that keep the agglomeration
    state in global memory (round per launch)."""
    tasks, refs = _tasks("global_state")
    _run(tasks, refs, _alone(sa, tasks), [dict(ONE_CHUNK, i0=0, i1=3, NS=1, gs=1, form=hb.FORM_SPLIT, max_n=4100, max_kpad=16, finish_at=15)])


def test_nested_batches(sa, monkeypatch):
    """The fallback list as three pipelined chunks, and from the progress callback the finished tasks again as NESTED batches (slot 2, own
    agglomeration scratch, one range, on the main stream while later chunks are in flight): tasks 0 - 1 and 2 - 3 come back a second time
    and equal the outer results bit for bit; the outer results equal those of the run without nested; task 4 (the last chunk is never
    reported by a callback) keeps the sentinel in the second set."""
    tasks, refs = _tasks("fallback")
    alone = _alone(sa, tasks)
    monkeypatch.setenv("SHARP_HC_CHUNK", "2")
    plain, _ = _batch(tasks)
    (outer, inner), plan = _batch(tasks, nested=True)
    piped = dict(pipe=1, NS=1, split=0, form=hb.FORM_1024, nested=0)
    inside = dict(i0=0, i1=2, slot=2, pipe=0, NS=1, split=0, form=hb.FORM_1024, nested=1, seq_deferred=0)
    _assert_plan(plan, [dict(piped, i0=0, i1=2, slot=0, seq_deferred=1), dict(piped, i0=2, i1=4, slot=1, seq_deferred=1),
                        dict(piped, i0=4, i1=5, slot=3, seq_deferred=0), inside, inside])
    (outer2, inner2), plan2 = _batch(tasks, nested=True)
    assert plan2 == plan
    _same_bits(outer, outer2)
    _same_bits(inner[:4], inner2[:4])
    _same_bits(outer, plain)
    _same_bits(outer[:4], inner[:4])
    for key in FLOATS + INTS:
        assert hb.is_sentinel(inner[4][key]).all(), key
    assert all(inner[4][key] == hb.INT_SENTINEL for key in SCALARS)
    for i, (t, r, r2, want, one) in enumerate(zip(tasks, outer, inner, refs, alone)):
        for got in (r, r2) if i < 4 else (r,):
            _no_sentinel(got)
            _vs_oracle(t, got, want)
            _vs_alone(t, got, one)
            assert got["sequential"] == ref.expected_sequential(t), i


def test_without_the_label_matrix(sa):
    """want_v = 0 with a null v: the same results, the label matrix left out (three tasks of different kinds, one with ties)."""
    tasks, _ = _tasks("interleaved")
    tasks = tasks[1:4] + tasks[5:]
    full = hb.get_opt_hclust_batch(list(tasks), want_v=True)
    lean = hb.get_opt_hclust_batch(list(tasks), want_v=False)
    assert all(r["v"] is None for r in lean)
    for a, b in zip(full, lean):
        for key in FLOATS:
            assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)), key
        assert np.array_equal(a["f"], b["f"]) and all(a[key] == b[key] for key in SCALARS)
        assert not hb.is_sentinel(b["f"]).any()


def test_nested_is_refused_beyond_four_tasks_per_compute_unit(sa, num_cu):
    t = ref.feature_task(8, 16, 2, 1, maxN=4)
    with pytest.raises(sa.SharpError, match="nested needs count"):
        hb.get_opt_hclust_batch([t] * (4 * num_cu + 1), nested=True)
    assert len(hb.get_opt_hclust_batch([t] * 2, nested=True)[0]) == 2


@pytest.mark.parametrize("bad,message", [(dict(n=2), "need at least 3 observations"), (dict(hmethod=9), "unknown agglomeration method"),
                                         (dict(minN=7, maxN=5), "empty range of cluster numbers"),
                                         (dict(N_cluster=30), "N.cluster must be smaller than the number of observations")])
def test_refusals_leave_the_library_usable(sa, bad, message):
    good = ref.feature_task(30, 16, 3, 31, maxN=8)
    kw = dict(maxN=8)
    kw.update({k: v for k, v in bad.items() if k != "n"})
    wrong = hb.make_task(good["mat"][: bad.get("n", 30)], **kw)
    with pytest.raises(sa.SharpError, match=message):
        hb.get_opt_hclust_batch([good, wrong, good])
    res = hb.get_opt_hclust_batch([good, good])
    want = ref.oracle_result(good)
    for r in res:
        _no_sentinel(r)
        assert np.array_equal(r["f"], want["f"]) and np.array_equal(r["v"], want["v"])
