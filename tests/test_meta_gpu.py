"""The meta-clustering stage (sharp_amd/csrc/meta.hip) tested DIRECTLY: wmetac_batch as a batch (sharp_wMetaC_batch: mixed tasks in one
call, running offsets, the per-task LDS split, the grow-only buffers, the vote on host threads), the weight and similarity kernels at the
shapes where they go wrong, the three rules of the host's vote, cluster_means_kernel and ensemble_mean_kernel on their own
(sharp_cluster_means, sharp_ensemble_mean), and the host logic of sMetaC (two-cluster override, k range by the number of cells) on
centroid tables of a few dozen rows.

Every wMetaC comparison (_vs_oracle) checks, in this order: allC; w1 against the exact rational weights within the bound derived from the
kernel's shape (_meta_ref.weight_rtol); S against the oracle at rtol 1e-12 / atol 1e-15, the same entries exactly 1, symmetric bit for
bit, unit diagonal, same-column pairs exactly 0, nothing above 1; tf, finalC, ncl and rc identical to the oracle's; x0 to 1e-15; no
sentinel inside what was written and the sentinel intact behind it.  No task is skipped: every task passes the margin check of
tests/_meta_ref.py (asserted on the CPU in tests/test_meta_cpu.py and again here)."""
import numpy as np
import pytest

import _meta_ref as ref
from sharp_amd import meta_batch as mb

pytestmark = pytest.mark.gpu

BITWISE = ("w1", "S", "x0")
EQUAL = ("tf", "finalC")
SCALARS = ("rc", "allC", "ncl")


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
    """a list, its oracle results, its exact weights, and the proof that every task of it can be compared exactly (never a skip)"""
    tasks, refs = ref.wm_reference(name)
    assert ref.wm_list_margin_failures(name) == []
    return tasks, refs, ref.wm_exact_weights(name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    """two results of one task: every double bit for bit, every integer equal"""
    for key in BITWISE:
        assert a[key].shape == b[key].shape and np.array_equal(_bits(a[key]), _bits(b[key])), key
    for key in EQUAL:
        assert np.array_equal(a[key], b[key]), key
    for key in SCALARS:
        assert a[key] == b[key], key


def _sentinels(out, N):
    """nothing of the sentinel inside what the batch wrote, nothing but the sentinel behind it"""
    used = mb.written(out, N)
    for key in mb.OUTPUTS:
        assert used[key] < out[key].size, key
        assert not mb.is_sentinel(out[key][: used[key]]).any(), f"{key}: a value was not written"
        assert mb.is_sentinel(out[key][used[key]:]).all(), f"{key}: written behind its extent"


def _vs_oracle(task, r, want, w_exact):
    N = task["labels"].shape[0]
    assert r["allC"] == want["allC"]
    np.testing.assert_allclose(r["w1"], w_exact, rtol=ref.weight_rtol(N), atol=0)
    S = r["S"]
    np.testing.assert_allclose(S, want["S"], rtol=1e-12, atol=1e-15)
    assert np.array_equal(S == 1.0, want["S"] == 1.0)
    assert np.array_equal(_bits(S), _bits(S.T))
    assert np.all(np.diag(S) == 1.0)
    _, allC, colof = ref.relabel(task["labels"])
    same = (colof[:, None] == colof[None, :]) & ~np.eye(allC, dtype=bool)
    assert np.all(_bits(S[same]) == 0)
    assert S.max() <= 1.0
    assert np.array_equal(r["tf"], want["tf"])
    assert np.array_equal(r["finalC"], want["finalC"])
    assert r["ncl"] == want["x0"].shape[1]
    assert r["rc"] == ref.expected_rc(want)
    assert r["x0"].shape == want["x0"].shape
    np.testing.assert_allclose(r["x0"], want["x0"], rtol=0, atol=1e-15)


def _batch(tasks):
    res, out = mb.wmetac_batch(list(tasks), raw=True)
    _sentinels(out, [t["labels"].shape[0] for t in tasks])
    return res


def _run(tasks, refs, weights):
    """one batch; every task against the oracle"""
    res = _batch(tasks)
    assert len(res) == len(tasks)
    for i, (t, r, want, w) in enumerate(zip(tasks, res, refs, weights)):
        try:
            _vs_oracle(t, r, want, w)
        except AssertionError as e:
            raise AssertionError(f"task {i} (N = {t['labels'].shape[0]}, C = {t['labels'].shape[1]}): {e}") from e
    return res


# ---- wmetac_batch as a batch --------------------------------------------------------------------------------------------------------
def test_mixed_tasks_in_one_call(sa):
    """N = 17, 2000, 63, 300, 1500, 65 with C = 2 .. 15 and allC = 6 .. 300 in ONE call: running offsets of short tasks behind long
    ones, grids sized by the largest task, the LDS split per task, the vote on 16 host threads.  Every task against the oracle, against
    itself sent alone (the batch changes no order of addition: bit for bit) and in the reversed list."""
    tasks, refs, weights = _tasks("mixed")
    res = _run(tasks, refs, weights)
    for i, t in enumerate(tasks):
        (one,) = _batch([t])
        try:
            _same_bits(res[i], one)
        except AssertionError as e:
            raise AssertionError(f"task {i} in the batch against the task alone: {e}") from e
    back = _batch(tasks[::-1])[::-1]
    for i, (a, b) in enumerate(zip(res, back)):
        try:
            _same_bits(a, b)
        except AssertionError as e:
            raise AssertionError(f"task {i} in the reversed batch: {e}") from e


def test_grow_only_buffers_hold_nothing_stale(sa):
    """a large batch, a batch of one task of 17 cells, the large batch again: the pinned label and member lists and the device buffers
    are reused; the third result is the first bit for bit"""
    tasks, refs, weights = _tasks("mixed")
    first = _batch(tasks)
    small = _batch(tasks[:1])
    third = _batch(tasks)
    _vs_oracle(tasks[0], small[0], refs[0], weights[0])
    for a, b in zip(first, third):
        _same_bits(a, b)
    _same_bits(small[0], first[0])


def test_small_and_ragged_numbers_of_cells(sa):
    """N = 2, 3, 15, 16, 17, 63, 64, 65: below one workgroup's 16 cells and around it, around a wave's 64 lanes; each alone (the grid the
    task's own N gives) and all in one batch"""
    tasks, refs, weights = _tasks("ragged")
    res = _run(tasks, refs, weights)
    for i, (t, want, w) in enumerate(zip(tasks, refs, weights)):
        (one,) = _run([t], [want], [w])
        _same_bits(one, res[i])


def test_label_block_at_the_lds_limit(sa):
    """C = 15: N = 5115 is the largest label block that fits the 150 KB the driver allows (both numbers derived from its formula); it
    matches the oracle.  One cell more is refused with the LDS message, nothing written."""
    C = 15
    N = ref.lds_largest_N(C)
    assert ref.lds_bytes(N, C) <= ref.LDS_LIMIT < ref.lds_bytes(N + 1, C)
    tasks, refs, weights = _tasks("lds_edge")
    assert tasks[0]["labels"].shape == (N, C)
    _run(tasks, refs, weights)
    over = ref.wm_task(ref.noisy_ensemble(N + 1, C, 8, 0.1, 2302), maxN=20)
    with pytest.raises(sa.SharpError, match="does not fit in LDS") as e:
        mb.wmetac_batch([ref.list_ragged()[3], over])
    assert all(mb.is_sentinel(a).all() for a in e.value.outputs.values())


def test_one_member_clusters(sa):
    """N = 200 with a column of 100 labels on two cells each and a column with 100 one-member clusters: allC = 212, member lists of
    length one and two"""
    tasks, refs, weights = _tasks("singletons")
    _run(tasks, refs, weights)


# ---- the vote on the host ---------------------------------------------------------------------------------------------------------------
def test_vote_ties_go_to_the_first_id_in_string_order(sa):
    """C = 2 with 14 meta-clusters: 33 - 39 cells per ensemble whose 1-1 tie the string order ("10" before "2") decides otherwise than
    the numeric order; C = 4: 2-2 ties.  Seven ensembles in one batch."""
    tasks, refs, weights = _tasks("vote_ties")
    assert min(ref.string_order_cells(t, r) for t, r in list(zip(tasks, refs))[:5]) >= 10
    _run(tasks, refs, weights)


def test_single_winner_fallback_and_the_missing_runner_up(sa):
    """Every cell's vote names one meta-cluster: the runner-up is taken where there is one.  First ensemble: half the cells have none and
    keep their vote, SHARP_WARN_NA_VOTE, x0 is 60 x 2.  Second (three constant columns, S == 1 throughout): all cells take the
    runner-up, rc 0."""
    tasks, refs, weights = _tasks("fallback")
    res = _run(tasks, refs, weights)
    assert res[0]["rc"] == mb.WARN_NA_VOTE and res[0]["tf"].tolist() == [1, 1, 1, 2] and res[0]["x0"].shape == (60, 2)
    assert res[0]["finalC"].tolist() == [1] * 30 + [2] * 30
    assert res[1]["rc"] == 0 and res[1]["tf"].tolist() == [1, 1, 2] and np.all(res[1]["finalC"] == 2) and res[1]["ncl"] == 1
    for i, t in enumerate(tasks):
        (one,) = _batch([t])
        _same_bits(one, res[i])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    good = ref.list_ragged()[4]
    return {
        "more than 65535 base clusters": (lambda: [good, ref.wm_task(np.arange(70000).reshape(-1, 1))], {}, "more than 65535 base clusters"),
        "two base clusters": (lambda: [good, ref.wm_task((np.arange(10) % 2).reshape(-1, 1))], {}, "fewer than 3 base clusters"),
        "one cell": (lambda: [good, ref.wm_task(np.array([[1, 2, 3]]))], {}, "empty label matrix"),
        "null labels": (lambda: [good], dict(null_labels=True), "empty label matrix"),
        "S too small": (lambda: [good, good], dict(cap=dict(S=2 * 25 - 1)), "output buffer is too small"),
        "finalC too small": (lambda: [good, good], dict(cap=dict(finalC=2 * 17 - 1)), "output buffer is too small"),
        "x0 too small": (lambda: [good], dict(cap=dict(x0=17 * 2 - 1)), "output buffer is too small"),
    }


@pytest.mark.parametrize("case", ["more than 65535 base clusters", "two base clusters", "one cell", "null labels", "S too small",
                                  "finalC too small", "x0 too small"])
def test_refusals_write_nothing_and_leave_the_library_usable(sa, case):
    """each with its message; every output keeps the sentinel over its whole capacity, also the good task's in front of the refused one"""
    build, kw, message = _refusal_cases()[case]
    with pytest.raises(sa.SharpError, match=message) as e:
        mb.wmetac_batch(build(), **kw)
    for key, a in e.value.outputs.items():
        assert a.size >= 1 and mb.is_sentinel(a).all(), key
    tasks, refs, weights = _tasks("ragged")
    _run(tasks[4:5], refs[4:5], weights[4:5])


# ---- cluster_means_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("p", ref.CM_P)
def test_cluster_means_on_their_own(sa, p, pad):
    """24 clusters of 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, ... members (a round of the 8 waves and a round of their four loads are the
    boundaries), the cells permuted; p on both sides of a 64-column slab; the rows laid out with ld = p and p + 3 (NaN between them).
    (a) small integers: every sum is exact, so the means equal the exact sum over the count bit for bit -- a member skipped or taken
    twice cannot hide; (b) mixed magnitudes and signs within the bound that follows the kernel's adds."""
    uid = ref.cm_uid()
    nC = len(ref.CM_SIZES)
    E = ref.cm_integer_E(p)
    out = mb.cluster_means(E, uid, nC, ld=p + pad)
    want = np.stack([E[uid == t].sum(0) / np.sum(uid == t) for t in range(nC)])
    assert np.array_equal(_bits(out[: nC * p].reshape(nC, p)), _bits(want))
    assert mb.is_sentinel(out[nC * p:]).all() and out.size > nC * p
    E = ref.cm_mixed_E(p)
    means, mag, cnt = ref.cm_mixed_ref(p)
    out = mb.cluster_means(E, uid, nC, ld=p + pad)
    got = out[: nC * p].reshape(nC, p)
    assert np.all(np.isfinite(got)) and mb.is_sentinel(out[nC * p:]).all()
    err = np.abs(got - means)
    tol = ref.cluster_means_atol(mag, cnt)
    assert np.all(err <= tol), (np.argwhere(err > tol)[:5], (err / tol).max())
    one = int(np.flatnonzero(cnt == 1)[0])
    assert np.array_equal(_bits(got[one]), _bits(E[uid == one][0]))          # the one-member cluster: its row


def test_cluster_means_refusals(sa):
    uid = ref.cm_uid()
    E = ref.cm_integer_E(1)
    with pytest.raises(sa.SharpError, match="uid out of range"):
        mb.cluster_means(E, uid, len(ref.CM_SIZES) - 1)
    with pytest.raises(sa.SharpError, match="a cluster without cells"):
        mb.cluster_means(E, uid, len(ref.CM_SIZES) + 1)
    with pytest.raises(sa.SharpError, match="bad sizes"):
        mb.cluster_means(E[:5], uid[:5], 6)


# ---- ensemble_mean_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one value", "ragged", "second trip of the grid"])
def test_ensemble_mean_is_the_same_sum_bit_for_bit(sa, num_cu, shape):
    """(sum over k ascending) / K in fp64: the kernel's order is the reference's, so every bit agrees.  The third shape has more values
    than the grid's CUs x 8 x 256 threads: the grid-stride loop takes a second trip."""
    threads = num_cu * 8 * 256
    n, p, K, ldE = {"one value": (1, 1, 1, 1), "ragged": (37, 50, 15, 750),
                    "second trip of the grid": (max(1100, threads // 500 + 52), 500, 3, 1508)}[shape]
    if shape == "second trip of the grid":
        assert threads < n * p < 2 * threads
    rng = np.random.default_rng(n + p)
    E = rng.standard_normal((n, K * p)) * 10.0 ** rng.uniform(-2, 2, (n, K * p))
    out = mb.ensemble_mean(E, K, p, ldE)
    assert np.array_equal(_bits(out[: n * p].reshape(n, p)), _bits(ref.ensemble_mean_ref(E, K, p)))
    assert mb.is_sentinel(out[n * p:]).all() and out.size > n * p


# ---- the host logic of sMetaC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ref.SM_OVERRIDE_SPREADS + (ref.SM_PLAIN_SPREAD,))
def test_smetac_two_cluster_override_on_24_centroids(sa, oracle, spread):
    """sharp_sMetaC on 696 cells in 24 labelled clusters of 1 .. 100 cells around two super-centres of three sub-centres each.  Sub-centre
    spread up to 0.5: the silhouette chooses two clusters by more than 0.05 and the override takes the second best level, 3 or 4; spread
    1.0: six, no override.  tf, finalColor and the row of the decision log, smetac_override_k included, against the oracle."""
    from test_decisions_gpu import F, compare_logs

    labels, E = ref.smetac_case(spread)
    want, rows = ref.smetac_reference(spread)
    sa.decision_log(True)
    try:
        got = sa.sMetaC(labels, E)
        log = sa.last_decisions()
    finally:
        sa.decision_log(False)
    assert np.array_equal(got["tf"], want["tf"]) and np.array_equal(got["finalColor"], want["finalColor"]) and got["warn"] == 0
    compare_logs(sa, log, rows, "sMetaC spread %g" % spread)
    assert log.shape[0] == 1
    if spread == ref.SM_PLAIN_SPREAD:
        assert log[0][F["chosen_k"]] == 6 and log[0][F["smetac_override_k"]] == 0
    else:
        assert log[0][F["chosen_k"]] == 2 and log[0][F["smetac_override_k"]] == got["tf"].max() and got["tf"].max() in (3, 4)


@pytest.mark.parametrize("ncells", ref.KR_NCELLS)
def test_k_range_rules_by_the_number_of_cells(sa, oracle, ncells):
    """One table of 60 centroid rows through sharp_unlimited_merge with the number of cells on both sides of every threshold of
    R/sMetaC.R:103-119 (10^4 steps of the lower bound, 10^5, 10^6): the oracle's answer is 3, then 9, 10, and from 10^6 cells on more than
    40 final clusters.  final_id and n_final identical to the oracle's."""
    from sharp_amd import device as dev

    M, cnt = ref.krange_table()
    want, _ = ref.krange_reference(ncells)
    fid, nf = dev.unlimited_merge(M, cnt, ncells)
    assert nf == want["n_final"] and np.array_equal(fid, want["final_id"])
