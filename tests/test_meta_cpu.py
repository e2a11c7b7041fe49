"""CPU checks behind tests/test_meta_gpu.py: the references of tests/_meta_ref.py pinned on the oracle, the margins of every task the GPU
file sends (none may be left out of an exact comparison there, so every one has to qualify here), the count of the property every case is
there for in the oracle's own result, and the packing of the Python wrapper of sharp_wMetaC_batch."""
import numpy as np
import pytest

import _hclust_batch_ref as hbref
import _meta_ref as ref
from sharp_amd import meta_batch as mb

F = {n: i for i, n in enumerate(("level", "block", "k", "fold", "n", "branch", "chosen_k", "ties", "best", "runner_up", "sil_minus_thre",
                                 "height_ratio", "smetac_override_k", "levels"))}


# ---- the references against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("mixed", 0), ("mixed", 1), ("mixed", 2), ("mixed", 3), ("mixed", 5), ("ragged", 0), ("ragged", 4),
                                        ("singletons", 0), ("vote_ties", 0), ("fallback", 0)])
def test_weights_and_similarity_references_agree_with_the_oracle(oracle, name, which):
    tasks, refs = ref.wm_reference(name)
    t, r = tasks[which], refs[which]
    N = t["labels"].shape[0]
    cid, allC, colof = ref.relabel(t["labels"])
    assert allC == r["allC"] == mb.base_clusters(t)
    # the oracle adds its N terms one after the other in double: N roundings, and a few for the terms and the epilogue
    w = ref.weights_exact(t["labels"])
    np.testing.assert_allclose(r["w1"], w, rtol=(N + 16) * 2.0 ** -53, atol=0)
    assert np.all(w > 0) and np.all(w <= 1.0)
    # the same set order and long-double sums as the oracle's: the quotients agree to the last bits, and exactly where they are 1
    S = ref.similarity_ref(t["labels"], r["w1"])
    np.testing.assert_allclose(S, r["S"], rtol=2.0 ** -51, atol=0)
    assert np.array_equal(S == 1.0, r["S"] == 1.0) and np.array_equal(S == 0.0, r["S"] == 0.0)
    same = colof[:, None] == colof[None, :]
    assert np.all(S[same & ~np.eye(allC, dtype=bool)] == 0.0) and np.all(np.diag(S) == 1.0) and np.array_equal(S, S.T)


def test_weight_tolerance_stays_below_the_pipeline_tests(oracle):
    """the derived bound, at the largest N that fits, is tighter than the rtol = 1e-13 tests/test_pipeline_gpu.py holds"""
    assert ref.weight_rtol(ref.lds_largest_N(15)) < 1e-13 and ref.weight_rtol(ref.lds_largest_N(1)) < 1e-12
    assert ref.weight_rtol(64) == 17 * 2.0 ** -53 and ref.weight_rtol(65) == 18 * 2.0 ** -53


def test_weight_integers_by_hand():
    """three cells, two columns: cells 0 and 1 together in both, cell 2 with cell 0 in neither and with cell 1 in neither"""
    lab = np.array([[1, 1], [1, 1], [2, 2]])
    assert ref.weight_integers(lab) == [0, 0, 0]              # cnt is 0 or C everywhere: no disagreement, w0 = 0
    assert np.array_equal(ref.weights_exact(lab), np.full(3, 0.01 / 1.01))
    lab = np.array([[1, 1], [1, 2], [2, 2]])                  # cnt: (0,1) 1, (0,2) 0, (1,2) 1 -> I = 1, 2, 1
    assert ref.weight_integers(lab) == [1, 2, 1]
    w0 = np.array([4 * 1, 4 * 2, 4 * 1]) / (3 * 4)
    np.testing.assert_allclose(ref.weights_exact(lab), (w0 + 0.01) / 1.01, rtol=4e-16)


def test_cluster_means_reference(oracle):
    uid = ref.cm_uid()
    assert sorted(np.bincount(uid)) == sorted(ref.CM_SIZES) and uid.size == 696 and uid[0] == 0
    assert all(np.any(np.diff(np.flatnonzero(uid == t)) > 1) for t in range(len(ref.CM_SIZES)) if np.sum(uid == t) > 1), "a contiguous cluster"
    first = [np.flatnonzero(uid == t)[0] for t in range(len(ref.CM_SIZES))]
    assert first == sorted(first)                             # first-appearance ids
    E = ref.cm_mixed_E(65)
    means, mag, cnt = ref.cm_mixed_ref(65)
    ld = E.astype(np.longdouble)
    for t in range(len(ref.CM_SIZES)):
        want = ld[uid == t].sum(0) / np.longdouble(cnt[t])
        assert np.all(np.abs(means[t] - want) <= 2.0 ** -52 * mag[t] / cnt[t])
    assert np.all(ref.cluster_means_atol(mag, cnt) > 0) and np.abs(E).max() / np.abs(E).min() > 1e6 and (E < 0).any() and (E > 0).any()
    # integers: any order of addition is exact
    Ei = ref.cm_integer_E(64)
    mi, magi, _ = ref.cluster_means_ref(Ei, uid)
    assert np.all(Ei == np.round(Ei)) and magi.max() < 2.0 ** 53
    for t in (0, 5, 10):
        assert np.array_equal(mi[t], Ei[uid == t].sum(0) / np.sum(uid == t))
    # the boundaries of the kernel's member split are among the sizes: one, a round of 8 waves, a round of 8 x 4 loads
    for s in (1, ref.CM_WAVES - 1, ref.CM_WAVES, ref.CM_WAVES + 1, 4 * ref.CM_WAVES - 1, 4 * ref.CM_WAVES, 4 * ref.CM_WAVES + 1):
        assert s in ref.CM_SIZES


def test_ensemble_mean_reference():
    rng = np.random.default_rng(1)
    E = rng.standard_normal((7, 12))
    got = ref.ensemble_mean_ref(E, 3, 4)
    assert np.array_equal(got, ((E[:, 0:4] + E[:, 4:8]) + E[:, 8:12]) / 3.0)
    assert np.array_equal(ref.ensemble_mean_ref(E[:, :4], 1, 4), E[:, :4])


# ---- every task can be demanded exactly, and holds what it was built for ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.WM_LISTS))
def test_every_wmetac_task_can_be_compared_exactly(oracle, name):
    assert ref.wm_list_margin_failures(name) == []
    tasks, refs = ref.wm_reference(name)
    for t, r in zip(tasks, refs):
        assert r["allC"] >= 3 and r["rc"] in (0, 4) and r["finalC"].size == t["labels"].shape[0] == r["x0"].shape[0]
        assert ref.lds_bytes(*t["labels"].shape) <= ref.LDS_LIMIT


def test_mixed_list_is_what_the_gpu_test_says(oracle):
    tasks, refs = ref.wm_reference("mixed")
    assert tuple(t["labels"].shape for t in tasks) == tuple((N, C) for N, C, _ in ref.MIXED_SHAPES)
    allC = [r["allC"] for r in refs]
    assert allC[4] > ref.SIM_STRIDE and max(allC[:4] + allC[5:]) < ref.SIM_STRIDE        # one task beyond a trip of the b loop
    assert len({t["maxN"] for t in tasks}) >= 4 and len({t["sil_thre"] for t in tasks}) >= 3
    assert [t["enN_cluster"] for t in tasks] == [0, 0, 0, 4, 0, 0] and refs[3]["tf"].max() == 4
    assert len(tasks) >= 4                                      # (the vote runs on 16 host threads from four tasks on)
    ns = [t["labels"].shape[0] for t in tasks]
    assert ns[0] < ns[1] > ns[2] and ns[0] % ref.WEIGHT_WAVES and ns[2] % ref.WEIGHT_WAVES   # short tasks around a long one, ragged


def test_ragged_and_edge_lists(oracle):
    tasks, refs = ref.wm_reference("ragged")
    assert tuple(t["labels"].shape[0] for t in tasks) == ref.RAGGED_N and tasks[0]["labels"].shape[1] == 3
    assert all(r["allC"] >= 3 for r in refs)
    # C = 15: the largest N is derived from the driver's formula; one more does not fit
    N = ref.lds_largest_N(15)
    assert ref.lds_bytes(N, 15) <= ref.LDS_LIMIT < ref.lds_bytes(N + 1, 15) and N == 5115
    (t,), (r,) = ref.wm_reference("lds_edge")
    assert t["labels"].shape == (N, 15)
    (t,), (r,) = ref.wm_reference("singletons")
    cid, allC, colof = ref.relabel(t["labels"])
    sizes = np.bincount(cid.ravel())
    assert t["labels"].shape[0] == 200 and np.unique(t["labels"][:, 1]).size == 100 and np.sum(sizes == 1) >= 100 and np.sum(sizes == 2) >= 100
    assert allC == r["allC"] > 200


def test_vote_ties_are_decided_by_string_order(oracle):
    tasks, refs = ref.wm_reference("vote_ties")
    two, four = list(zip(tasks, refs))[:5], list(zip(tasks, refs))[5:]
    for t, r in two + four:
        assert r["tf"].max() == 14                               # ids 10 .. 14 sort before 2 .. 9 as strings
    counts = [ref.string_order_cells(t, r) for t, r in two]
    assert min(counts) >= 10, counts
    assert all(t["labels"].shape[1] == 4 for t, _ in four) and sum(ref.string_order_cells(t, r) for t, r in four) >= 1
    # sorting the ties numerically would change finalC in just those cells
    t, r = two[0]
    cid, _, _ = ref.relabel(t["labels"])
    votes = r["tf"][cid]
    numeric = np.array([min(v) if v[0] != v[1] else v[0] for v in votes])
    assert np.sum(numeric != r["finalC"]) == counts[0]


def test_fallback_cases(oracle):
    (a, b), (ra, rb) = ref.wm_reference("fallback")
    assert ra["tf"].tolist() == [1, 1, 1, 2] and set(ra["finalC"]) == {1, 2} and ra["rc"] == 4 and ra["x0"].shape == (60, 2)
    assert ref.expected_rc(ra) == mb.WARN_NA_VOTE
    assert ra["finalC"].tolist() == [1] * 30 + [2] * 30
    assert rb["tf"].tolist() == [1, 1, 2] and np.all(rb["finalC"] == 2) and rb["rc"] == 0 and ref.expected_rc(rb) == 0
    # the second: S is one throughout, which is why its decision is exact without margins (wm_margin_failures)
    assert np.all(rb["S"] == 1.0)
    t = ref.hclust_task_of(b, rb)
    h = hbref.oracle_result(t)
    assert np.all(h["height"] == 0.0) and h["msil"].size == 1


# ---- sMetaC and the k-range rules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ref.SM_OVERRIDE_SPREADS + (ref.SM_PLAIN_SPREAD,))
def test_smetac_cases_decide_as_planned_with_margins(oracle, spread):
    labels, E = ref.smetac_case(spread)
    res, rows = ref.smetac_reference(spread)
    assert rows.shape == (1, 14) and res["rc"] == 0 and res["nC"] == len(ref.CM_SIZES) and labels.size == 696 and E.shape == (696, ref.SM_P)
    row = rows[0]
    means, _, _ = ref.cluster_means_ref(E, ref.cm_uid())
    task = ref.smetac_hclust_task(means, labels.size)
    want = hbref.oracle_result(task)
    assert hbref.check_margins(task, want) == [] and (task["minN"], task["maxN"]) == (2, 40)
    assert row[F["branch"]] == 0 and row[F["ties"]] == 1 and row[F["chosen_k"]] == want["optN"]
    top = np.sort(want["msil"])[::-1]
    if spread == ref.SM_PLAIN_SPREAD:
        assert row[F["chosen_k"]] == 6 and row[F["smetac_override_k"]] == 0 and res["tf"].max() == 6
        assert np.array_equal(res["tf"], want["f"]) and top[0] - top[1] > 1e-3
    else:
        assert row[F["chosen_k"]] == 2 and row[F["best"]] - row[F["runner_up"]] > 0.05
        assert row[F["smetac_override_k"]] in (3, 4) and res["tf"].max() == row[F["smetac_override_k"]]
        assert top[1] - top[2] > 1e-6, "the override's own choice (the second largest median silhouette) has no margin"
        k = int(row[F["smetac_override_k"]])
        assert np.array_equal(res["tf"], want["v"][:, k - task["minN"]])
    assert np.array_equal(res["finalColor"], res["tf"][ref.cm_uid()])


def test_krange_rules_change_the_oracles_answer_with_margins(oracle):
    M, cnt = ref.krange_table()
    assert M.shape[0] == 60 and cnt.size == 60 and (cnt < 10).sum() == 4
    finals, ranges = [], []
    for ncells in ref.KR_NCELLS:
        res, rows = ref.krange_reference(ncells)
        assert rows.shape == (1, 14) and rows[0][F["level"]] == 3 and res["rc"] == 0
        task = ref.smetac_hclust_task(M, ncells, 2, max(40, -(-ncells // 5000)))
        want = hbref.oracle_result(task)
        assert hbref.check_margins(task, want) == [], ncells
        assert rows[0][F["levels"]] == want["msil"].size and rows[0][F["chosen_k"]] == want["optN"] and rows[0][F["smetac_override_k"]] == 0
        # the log's own margins: one maximum, its runner-up more than 1e-8 relative below, max(msil) away from sil.thre
        best, second = rows[0][F["best"]], rows[0][F["runner_up"]]
        assert rows[0][F["ties"]] == 1 and best - second > 1e-8 * abs(best) and abs(rows[0][F["sil_minus_thre"]]) > 1e-8, ncells
        finals.append(res["n_final"])
        ranges.append((task["minN"], task["maxN"]))
    assert ranges == [(2, 40), (2, 40), (2, 40), (3, 40), (9, 40), (10, 40), (10, 200), (20, 200), (30, 300)]
    assert finals[:4] == [3, 3, 3, 3] and finals[4] == 9 and finals[5] == finals[6] == 10 and finals[7] == finals[8] > 40
    assert ref.krange(9999, 60, 2, 40) == (2, 40) and ref.krange(10 ** 6, 60, 2, 200) == (20, 200) and ref.krange(50000, 7, 2, 40) == (2, 40)


# ---- the wrapper's packing ------------------------------------------------------------------------------------------------------------
def test_pack_capacities_and_unpack():
    tasks = [mb.make_task(np.array([[1, 5], [2, 5], [1, 6]]), maxN=7, sil_thre=0.1), mb.make_task(np.arange(8).reshape(4, 2) % 3, hmethod="average",
                                                                                                   enN_cluster=2, minN=3, height_Ntimes=1.5)]
    a = mb.pack_tasks(tasks)
    assert a["N"].tolist() == [3, 4] and a["C"].tolist() == [2, 2] and a["hmethod"].tolist() == [1, 4] and a["enN_cluster"].tolist() == [0, 2]
    assert a["minN"].tolist() == [2, 3] and a["maxN"].tolist() == [7, 40] and a["sil_thre"].tolist() == [0.1, 0.35]
    assert a["labels"].dtype == np.int32 and a["labels"].tolist() == [1, 2, 1, 5, 5, 6, 0, 2, 1, 0, 1, 0, 2, 1]      # column-major, task after task
    assert [mb.base_clusters(t) for t in tasks] == [4, 6]
    cap = mb.capacities(tasks, pad=0)
    assert cap == dict(rc=2, allC=2, ncl=2, finalC=7, w1=7, S=16 + 36, tf=10, x0=3 * 3 + 4 * 2)
    assert mb.capacities(tasks)["S"] == 52 + mb.PAD
    with pytest.raises(TypeError):
        mb.make_task(np.zeros((3, 2)))
    out = mb.alloc_outputs(mb.capacities(tasks))
    assert out["S"].dtype == out["x0"].dtype == out["w1"].dtype == np.float64 and out["tf"].dtype == out["rc"].dtype == np.int32
    rng = np.random.default_rng(2)
    for key in out:
        out[key][...] = rng.integers(1, 1000, out[key].size)
    out["allC"][:2] = [4, 6]
    out["ncl"][:2] = [2, 1]
    res = mb.unpack_results(out, a["N"])
    assert mb.written(out, a["N"]) == dict(rc=2, allC=2, ncl=2, finalC=7, w1=7, S=52, tf=10, x0=3 * 2 + 4 * 1)
    assert res[0]["S"].shape == (4, 4) and res[1]["S"].shape == (6, 6) and np.array_equal(res[1]["S"].ravel(), out["S"][16:52])
    assert np.array_equal(res[0]["finalC"], out["finalC"][:3]) and np.array_equal(res[1]["w1"], out["w1"][3:7])
    assert np.array_equal(res[1]["tf"], out["tf"][4:10]) and res[0]["x0"].shape == (3, 2) and res[1]["x0"].shape == (4, 1)
    assert np.array_equal(res[0]["x0"].T.ravel(), out["x0"][:6]) and np.array_equal(res[1]["x0"][:, 0], out["x0"][6:10])
    # more base clusters than the driver takes: no room is asked for what it will refuse to compute
    big = mb.make_task(np.arange(70000).reshape(-1, 1))
    cap = mb.capacities([big], pad=1)
    assert mb.base_clusters(big) > mb.MAX_BASE_CLUSTERS and cap["S"] == cap["tf"] == cap["x0"] == 1 and cap["finalC"] == 70001
