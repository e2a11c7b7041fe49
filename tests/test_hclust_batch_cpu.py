"""CPU checks behind tests/test_hclust_batch_gpu.py: the task generators, the margins of every task list the GPU file uses (no task may be
left out of an exact comparison there, so every one has to qualify here), and the packing of the Python wrapper of
sharp_get_opt_hclust_batch."""
import numpy as np
import pytest

import _hclust_batch_ref as ref
from sharp_amd import hclust_batch as hb


def test_generators_are_deterministic_and_shaped_as_stated(oracle):
    a, b = ref.gaussian_mixture(50, 16, 3, 7), ref.gaussian_mixture(50, 16, 3, 7)
    assert np.array_equal(a, b) and a.shape == (50, 16) and not np.array_equal(a, ref.gaussian_mixture(50, 16, 3, 8))
    s = ref.similarity_task(40, 20, 3, 9)
    assert s["kind"] == hb.SIMILARITY and np.array_equal(s["mat"], s["mat"].T) and np.all(np.diag(s["mat"]) == 1.0)
    assert np.abs(s["mat"]).max() <= 1.0
    w = ref.wmetac_similarity_task(200, 4, 5, 10)
    assert w["kind"] == hb.SIMILARITY and np.array_equal(w["mat"], w["mat"].T) and w["mat"].shape[0] == w["mat"].shape[1] >= 5
    sat = ref.saturated_similarity_task(300, 6, 1306)
    off = sat["mat"][~np.eye(sat["mat"].shape[0], dtype=bool)]
    assert np.any(off == 1.0)                                     # exact ones off the diagonal
    r = ref.oracle_result(sat)
    assert np.sum(r["msil"] == r["msil"].max()) >= 2, "the saturated task has no tied maximum of msil"
    t = ref.tie_task(60, 16, 3, 11, 10, maxN=20)
    assert t["tie"] and np.array_equal(t["mat"][50:], t["mat"][:10]) and t["mat"].shape[0] >= 2 * t["maxN"]
    assert ref.expected_sequential(t) == 1
    assert ref.expected_sequential(ref.feature_task(30, 16, 2, 1, hmethod="median")) == 1
    assert ref.expected_sequential(ref.feature_task(30, 16, 2, 1, hmethod="single")) == 0


def test_task_lists_are_what_the_gpu_tests_say():
    assert [t["mat"].shape[0] for t in ref.list_mixed_sizes()] == [1000, 3, 40, 127, 128, 129, 300, 999]
    assert sorted(t["hmethod"] for t in ref.list_linkages()) == sorted(ref.REDUCIBLE + ref.NOT_REDUCIBLE)
    assert [t["kind"] for t in ref.list_interleaved()] == [0, 1, 1, 0, 1, 1]
    assert len({t["mat"].shape[0] for t in ref.list_interleaved()}) == 6
    assert [(t["mat"].shape[0], t["kind"]) for t in ref.list_nn_parts()] == [(2049, 0), (300, 0), (200, 1), (2048, 0)]
    assert [t["maxN"] for t in ref.list_kpad()] == [15, 16, 17, 40, 64, 70]
    assert [hb.nk_of(t) for t in ref.list_many_levels()] == [30, 3, 1, 3]
    short = ref.list_given_and_short()[2]
    assert short["mat"].shape[0] == 12 and short["maxN"] == 40 and hb.nk_of(short) == 10
    assert [t["tie"] for t in ref.list_fallback()] == [False, True, False, True, False]
    two = ref.list_two_ranges()
    assert len(two) == ref.K_TWO_RANGES_TASKS and [i for i, t in enumerate(two) if t["tie"]] == [0, 96, 97, 150, 193]
    ns = [t["mat"].shape[0] for t in two]
    assert min(ns) >= 24 and max(ns) <= 60 and len(set(ns)) > 10 and all(t["mat"].shape[1] == 16 and t["maxN"] <= 8 for t in two)
    assert [i for i, t in enumerate(ref.list_three_ranges()) if t["tie"]] == [3]
    for count in (257, 300, 513):
        many = ref.list_many(count)
        assert len(many) == count and 4 <= sum(t["tie"] for t in many) <= 6
    assert [t["mat"].shape[0] for t in ref.list_global_state()] == [4100, 50, 1000]
    # the driver's thresholds that the lists are sized by (the GPU tests assert the plan that follows from them)
    rup = lambda v, a: -(-v // a) * a      # noqa: E731
    ns = [t["mat"].shape[0] for t in ref.list_mixed_sizes()]
    assert len(ns) <= ref.K_SPLIT_MAX_TASKS and max(ns) == ref.K_SPLIT_MIN_OBS and sorted(ns)[-2] == ref.K_SPLIT_MIN_OBS - 1
    assert max(t["mat"].shape[0] for t in ref.list_linkages() + ref.list_interleaved() + ref.list_fallback()) < ref.K_SPLIT_MIN_OBS
    assert rup(2049, 128) > ref.NN_PARTS_MAX_NLD == rup(2048, 128)
    assert rup(64, 16) == ref.LANE_MAX_KPAD < rup(70, 16)
    assert ref.list_global_state()[0]["mat"].shape[0] > ref.HR_MAXN > ref.list_global_state()[2]["mat"].shape[0]
    assert ref.NUM_CU < 257 and ref.NUM_CU < 300 and 513 > 2 * ref.NUM_CU
    for name, build in ref.ALL_LISTS.items():                    # duplicated rows only where no candidate level cuts through them
        assert all(t["mat"].shape[0] >= 2 * t["maxN"] for t in build() if t["tie"] and not t.get("saturated")), name


@pytest.mark.parametrize("name", sorted(ref.ALL_LISTS))
def test_every_task_of_every_list_can_be_compared_exactly(oracle, name):
    assert ref.margin_failures(name) == []
    tasks, refs = ref.reference(name)
    assert len(tasks) == len(refs) and all(r["f"].size == t["mat"].shape[0] for t, r in zip(tasks, refs))
    assert all(r["msil"].size == hb.nk_of(t) for t, r in zip(tasks, refs))


def test_check_margins_refuses_what_it_should(oracle):
    t = ref.feature_task(80, 20, 3, 21, maxN=10)
    good = ref.oracle_result(t)
    assert ref.check_margins(t, good) == []
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    top = int(np.argmax(r["msil"]))
    r["msil"][(top + 1) % r["msil"].size] = r["msil"][top] * (1 - 1e-9)          # a runner-up within 1e-8
    assert any("msil" in w for w in ref.check_margins(t, r))
    r["msil"][(top + 1) % r["msil"].size] = r["msil"][top]                       # an exact tie is allowed
    assert ref.check_margins(t, r) == []
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    r["height"][-3] = r["height"][-2] * (1 - 1e-10)                              # two of the last merges at (almost) one height
    assert any("heights" in w for w in ref.check_margins(t, r))
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    thr = dict(t, sil_thre=float(r["msil"].max()) - 1e-9)
    assert any("threshold" in w for w in ref.check_margins(thr, r))


def _fake_outputs(n, nk, want_v, sets, seed):
    rng = np.random.default_rng(seed)
    out = hb.alloc_outputs(n, nk, want_v, sets)
    for key, a in out.items():
        if a is not None:
            a[...] = rng.integers(1, 1 << 20, a.size).astype(a.dtype)
    return out


@pytest.mark.parametrize("want_v", [True, False])
@pytest.mark.parametrize("sets", [1, 2])
def test_pack_then_unpack_gives_the_same_arrays(want_v, sets):
    """ragged n and nk: every value of every output array belongs to exactly one task of one set, at the offsets the header states"""
    tasks = [hb.make_task(np.full((n, p), 100.0 * i) + np.arange(n * p).reshape(n, p), kind, hmethod=hm, N_cluster=ncl, minN=mn, maxN=mx,
                          sil_thre=0.1 * i, height_Ntimes=1.5 + i)
             for i, (n, p, kind, hm, ncl, mn, mx) in enumerate([(5, 3, 0, "ward.D", 0, 2, 40), (12, 12, 1, "single", 0, 3, 7), (3, 2, 0, 8, 0, 2, 40),
                                                                 (9, 4, 0, "median", 4, 2, 40), (7, 7, 1, "average", 0, 2, 3)])]
    a = hb.pack_tasks(tasks)
    assert a["n"].tolist() == [5, 12, 3, 9, 7] and a["p"].tolist() == [3, 12, 2, 4, 7] and a["kind"].tolist() == [0, 1, 0, 0, 1]
    assert a["hmethod"].tolist() == [1, 2, 8, 6, 4] and a["N_cluster"].tolist() == [0, 0, 0, 4, 0]
    assert a["minN"].tolist() == [2, 3, 2, 2, 2] and a["maxN"].tolist() == [40, 7, 40, 40, 3]
    assert all(a[k].dtype == np.int32 for k in ("n", "p", "kind", "hmethod", "N_cluster", "minN", "maxN"))
    assert a["sil_thre"].dtype == a["height_Ntimes"].dtype == a["mats"].dtype == np.float64
    o = 0
    for t in tasks:                                              # the matrices one after the other, row-major
        assert np.array_equal(a["mats"][o: o + t["mat"].size].reshape(t["mat"].shape), t["mat"])
        o += t["mat"].size
    assert o == a["mats"].size
    nk = np.array([hb.nk_of(t) for t in tasks])
    assert nk.tolist() == [3, 5, 1, 1, 2]
    lay = hb.output_layout(a["n"], nk)
    assert lay["f"].tolist() == [0, 5, 17, 20, 29, 36] and lay["k"].tolist() == [0, 3, 8, 9, 10, 12]
    assert lay["v"].tolist() == [0, 15, 75, 78, 87, 101] and lay["h"].tolist() == [0, 4, 15, 17, 25, 31]
    out = _fake_outputs(a["n"], nk, want_v, sets, 3)
    assert out["f"].size == sets * 36 and out["msil"].size == out["CHind"].size == sets * 12 and out["height"].size == sets * 31
    assert (out["v"].size == sets * 101) if want_v else out["v"] is None
    again = {k: (np.zeros_like(v) if v is not None else None) for k, v in out.items()}
    for which in range(sets):
        res = hb.unpack_results(out, a["n"], nk, want_v, which)
        assert len(res) == 5
        for t, r in enumerate(res):                              # put every piece back where the layout says it came from
            assert r["f"].size == a["n"][t] and r["msil"].size == r["CHind"].size == nk[t] and r["height"].size == a["n"][t] - 1
            again["f"][which * 36 + lay["f"][t]: which * 36 + lay["f"][t + 1]] = r["f"]
            again["msil"][which * 12 + lay["k"][t]: which * 12 + lay["k"][t + 1]] = r["msil"]
            again["CHind"][which * 12 + lay["k"][t]: which * 12 + lay["k"][t + 1]] = r["CHind"]
            again["height"][which * 31 + lay["h"][t]: which * 31 + lay["h"][t + 1]] = r["height"]
            if want_v:
                assert r["v"].shape == (a["n"][t], nk[t])
                again["v"][which * 101 + lay["v"][t]: which * 101 + lay["v"][t + 1]] = r["v"].T.ravel()    # level-major in the array
            else:
                assert r["v"] is None
            for key in ("optN", "nk", "branch", "rc", "sequential"):
                again[key][which * 5 + t] = r[key]
    for key, v in out.items():
        assert (v is None and again[key] is None) or np.array_equal(v, again[key]), key


def test_sentinels_are_told_apart():
    d = np.array([np.nan, 1.0, 0.0])
    d.view(np.uint64)[2] = hb.NAN_SENTINEL_BITS
    assert hb.is_sentinel(d).tolist() == [False, False, True]     # (an ordinary NaN is not the sentinel)
    assert hb.is_sentinel(np.array([0, hb.INT_SENTINEL, -1], np.int32)).tolist() == [False, True, False]
    assert len(hb.PLAN_COLUMNS) == 16
