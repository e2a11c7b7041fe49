"""CPU side of the meta-clustering tests (tests/test_meta_gpu.py, tests/test_meta_cpu.py): plain references of what the kernels of
sharp_amd/csrc/meta.hip compute, the ensembles and centroid tables the GPU tests send, and for every one of them the proof -- from the
oracle's numbers alone -- that the oracle's decision can be demanded exactly of another implementation.

References (pinned on the oracle by test_meta_cpu.py):
  weights_exact       w1 of wMetaC from the exact rational 4 I_i / (N C^2), I_i = sum_j cnt_ij (C - cnt_ij) in Python integers
  similarity_ref      S of wMetaC: sum(w1[a n b]) / sum(w1[a u b]) in R's set order, long-double sums
  cluster_means_ref   exactly rounded column sums (math.fsum) over the count
  ensemble_mean_ref   numpy fp64, k ascending, one division: the kernel's own order, so the comparison is bit for bit

Every wMetaC task here is built from fixed seeds and passes _hclust_batch_ref.check_margins on the get_opt_hclust task made of the
oracle's S; test_meta_cpu.py asserts that, and that the property a case is there for really occurs in the oracle's result.  No task is
ever left out on the GPU side: a builder that fails its margin gets another seed HERE."""
import functools
import math

import numpy as np

import _hclust_batch_ref as hbref
from sharp_amd import meta_batch as mb
from sharp_amd.hclust_batch import SIMILARITY
from sharp_amd.hclust_batch import make_task as make_hc_task

LDS_LIMIT = 150 * 1024             # meta.hip, wmetac_batch: the label block and the table of one task
WEIGHT_WAVES = 16                  # meta.hip, WW_THREADS / 64: cells per workgroup of wm_weights_kernel
SIM_STRIDE = 256                   # meta.hip, wm_similarity_kernel: b advances by the workgroup's 256 threads
CM_WAVES = 8                       # meta.hip, cluster_means_kernel: members round-robin over 8 waves, four loads each


def _oracle():
    return hbref._oracle()


# ---- references ----------------------------------------------------------------------------------------------------------------------

def relabel(nC):
    """global base-cluster ids as R's unique(x) numbers them: column after column, by first appearance inside a column.
    -> cid (N, C), allC, colof (allC)"""
    nC = np.asarray(nC)
    N, C = nC.shape
    cid = np.zeros((N, C), np.int64)
    colof = []
    allC = 0
    for c in range(C):
        _, first, inv = np.unique(nC[:, c], return_index=True, return_inverse=True)
        rank = np.empty(first.size, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(first.size)
        cid[:, c] = allC + rank[inv.ravel()]
        colof += [c] * first.size
        allC += first.size
    return cid, allC, np.array(colof)


def weight_integers(nC):
    """I_i = sum_j cnt_ij (C - cnt_ij), cnt_ij = the number of columns that put i and j together: Python integers"""
    nC = np.asarray(nC)
    N, C = nC.shape
    out = np.zeros(N, np.int64)
    for i0 in range(0, N, 512):                                      # (N x N counts in strips)
        cnt = np.zeros((min(512, N - i0), N), np.int64)
        for c in range(C):
            cnt += nC[i0: i0 + 512, c][:, None] == nC[None, :, c]
        out[i0: i0 + 512] = (cnt * (C - cnt)).sum(1)
    return [int(v) for v in out]


def weights_exact(nC):
    """w1 = (w0 + 0.01) / 1.01 with w0 = 4 I / (N C^2) exact: the quotient of two integers rounded once to long double, then R's two
    operations on it in long double (0.01 is R's double constant).  -> float64, the long-double value rounded"""
    N, C = np.asarray(nC).shape
    LD = np.longdouble
    w0 = np.array([LD(4 * v) for v in weight_integers(nC)], LD) / LD(N * C * C)
    return ((w0 + LD(0.01)) / (LD(1) + LD(0.01))).astype(np.float64)


def weight_rtol(N):
    """The relative error bound of wm_weights_kernel against weights_exact, from the kernel's shape; every term is non-negative, so each
    rounding adds at most 2^-53 relative to the sum it rounds:
      a lane's chain           ceil(N / 64) adds of table entries
      the wave's combination   6 shuffle adds
      a table entry            3 roundings (q / C, 1 - x, x (1 - x))
      the epilogue             4 scalar operations (4 / N, times the sum, + 0.01, / 1.01), and 1 + 0.01 rounded
    = ceil(N / 64) + 14, taken as + 16 for the second-order terms and the reference's own long-double roundings."""
    return (-(-N // 64) + 16) * 2.0 ** -53


def similarity_ref(nC, w1):
    """S[a][b] = sum(w1[a n b]) / sum(w1[a u b]) (R/wMetaC.R:70-77, getss): the intersection in the order of a's cells, the union as a's
    cells then b's cells not in a, each summed from the left in long double; same-column pairs 0, the diagonal 1"""
    cid, allC, colof = relabel(nC)
    w = np.asarray(w1, np.float64).astype(np.longdouble)
    mem = [np.flatnonzero(cid[:, colof[a]] == a) for a in range(allC)]
    left = lambda v: np.add.accumulate(v)[-1] if v.size else np.longdouble(0)   # noqa: E731
    S = np.zeros((allC, allC))
    for a in range(allC):
        S[a, a] = 1.0
        wa = left(w[mem[a]])
        for b in range(a + 1, allC):
            if colof[a] == colof[b]:
                continue
            both = mem[a][cid[mem[a], colof[b]] == b]
            if both.size:
                rest = mem[b][cid[mem[b], colof[a]] != a]
                uni = np.add.accumulate(np.concatenate([[wa], w[rest]]))[-1]
                S[a, b] = S[b, a] = float(left(w[both]) / uni)
    return S


def cluster_means_ref(E, uid):
    """-> (means, sum |x| per entry, counts): the exactly rounded sum of every cluster's column (math.fsum) over its count"""
    E = np.asarray(E, np.float64)
    uid = np.asarray(uid)
    nC, p = int(uid.max()) + 1, E.shape[1]
    means, mag, cnt = np.zeros((nC, p)), np.zeros((nC, p)), np.zeros(nC, np.int64)
    for t in range(nC):
        rows = E[uid == t]
        cnt[t] = rows.shape[0]
        for c in range(p):
            means[t, c] = math.fsum(rows[:, c]) / rows.shape[0]
            mag[t, c] = math.fsum(np.abs(rows[:, c]))
    return means, mag, cnt


def cluster_means_atol(mag, cnt):
    """The absolute bound per entry of cluster_means_kernel against cluster_means_ref, along the kernel's adds: an accumulator takes every
    32nd member, a chain of ceil(cnt / 32) adds; two pair adds join a wave's four accumulators; eight partial sums are added; one
    division; the reference rounds its sum and its quotient once each -> (ceil(cnt / 32) + 12) 2^-53 sum|x| / cnt"""
    cnt = np.asarray(cnt, np.float64)[:, None]
    return (np.ceil(cnt / 32) + 12) * 2.0 ** -53 * mag / cnt


def ensemble_mean_ref(E, K, p):
    E = np.asarray(E, np.float64)
    s = np.zeros((E.shape[0], p))
    for k in range(K):
        s = s + E[:, k * p: (k + 1) * p]
    return s / float(K)


# ---- ensembles -------------------------------------------------------------------------------------------------------------------------

def noisy_ensemble(N, C, G, flip, seed):
    """as tests/test_pipeline_gpu.py builds them: renamed copies of one partition, a share `flip` of every column redrawn"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, G + 1, N)
    cols = []
    for c in range(C):
        col = (base + c) % G + 1
        f = rng.random(N) < flip
        col[f] = rng.integers(1, G + 1, f.sum())
        cols.append(col)
    return np.stack(cols, 1)


def wm_task(labels, **kw):
    return mb.make_task(labels, **kw)


def oracle_wmetac(task):
    r = _oracle().wMetaC(task["labels"], hmethod=task["hmethod"], enN=task["enN_cluster"], minN=task["minN"], maxN=task["maxN"],
                         sil_thre=task["sil_thre"], height_Ntimes=task["height_Ntimes"])
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def hclust_task_of(task, ref):
    """the get_opt_hclust task inside a wMetaC task, from the oracle's S.  S holds exact zeros and ones, so equal distances and equal
    heights occur: the agglomeration resolves those in R's order (the sequential kernel), which check_margins lets pass as exact ties."""
    t = make_hc_task(ref["S"], SIMILARITY, hmethod=task["hmethod"], N_cluster=task["enN_cluster"], minN=task["minN"], maxN=task["maxN"],
                     sil_thre=task["sil_thre"], height_Ntimes=task["height_Ntimes"])
    t["tie"] = True
    return t


def wm_margin_failures(task, ref):
    """An ensemble of constant columns has S == 1 throughout: every distance and every height is exactly zero and the statistics are
    exact zeros or NaN, so each comparison on the way to the decision is between exact values -- nothing that rounding could turn."""
    if np.all(ref["S"] == 1.0):
        return []
    t = hclust_task_of(task, ref)
    return hbref.check_margins(t, hbref.oracle_result(t))


def expected_rc(ref):
    """the oracle's warning bits as the library's (SHARP_WARN_RANGE 16 for the oracle's 2, SHARP_WARN_NA_VOTE 32 for its 4)"""
    return (mb.WARN_RANGE if ref["rc"] & 2 else 0) | (mb.WARN_NA_VOTE if ref["rc"] & 4 else 0)


def lds_bytes(N, C):
    """wmetac_batch: the uint16 label block rounded up to 16 bytes, and C + 1 doubles"""
    return -(-N * C * 2 // 16) * 16 + (C + 1) * 8


def lds_largest_N(C):
    N = LDS_LIMIT // (2 * C)
    while lds_bytes(N, C) > LDS_LIMIT:
        N -= 1
    while lds_bytes(N + 1, C) <= LDS_LIMIT:
        N += 1
    return N


def _cached(fn):
    return functools.lru_cache(maxsize=None)(fn)


MIXED_SHAPES = ((17, 2, 3), (2000, 15, 12), (63, 5, 4), (300, 3, 6), (1500, 3, 100), (65, 4, 5))


@_cached
def list_mixed():
    """one call: short tasks behind long ones, allC from 6 to about 300 (> 256: a second trip of the similarity kernel's b loop),
    different maxN and sil_thre, one task with the number of meta-clusters given"""
    kws = (dict(maxN=40, sil_thre=0.35), dict(maxN=20, sil_thre=0.3), dict(maxN=12, sil_thre=0.35), dict(maxN=40, sil_thre=0.2, enN_cluster=4),
           dict(maxN=150, sil_thre=0.35), dict(maxN=9, sil_thre=0.4))
    seeds = (2101, 2102, 2103, 2104, 2105, 2106)
    flips = (0.1, 0.15, 0.1, 0.05, 0.05, 0.1)
    return tuple(wm_task(noisy_ensemble(N, C, G, f, s), **kw) for (N, C, G), f, s, kw in zip(MIXED_SHAPES, flips, seeds, kws))


RAGGED_N = (2, 3, 15, 16, 17, 63, 64, 65)


@_cached
def list_ragged():
    """N around the 16 cells of a workgroup and the 64 lanes of a wave, and N = 2"""
    out = []
    for N in RAGGED_N:
        i = np.arange(N)
        cols = [i % 2, i % 2, i % 2] if N == 2 else [i % 2, i % 3]
        out.append(wm_task(np.stack(cols, 1) + 1))
    return tuple(out)


@_cached
def list_lds_edge():
    """C = 15 and the largest N whose label block fits in LDS"""
    return (wm_task(noisy_ensemble(lds_largest_N(15), 15, 8, 0.1, 2301), maxN=20),)


@_cached
def list_singletons():
    """N = 200: one column with 100 distinct labels (each on two cells), one with every cell a cluster of its own among 100 cells,
    beside two ordinary columns"""
    rng = np.random.default_rng(2401)
    N = 200
    base = rng.integers(1, 5, N)
    pairs = rng.permutation(N) // 2 + 1                                # N / 2 distinct labels
    lone = np.where(np.arange(N) < 100, np.arange(N) + 1, 1000 + base)  # 100 one-member clusters, the rest by the partition
    noisy = base.copy()
    f = rng.random(N) < 0.05
    noisy[f] = rng.integers(1, 5, f.sum())
    return (wm_task(np.stack([base, pairs, rng.permutation(lone), noisy], 1), maxN=40),)


TIE_SEEDS = (1, 2, 3, 4, 5)


@_cached
def list_vote_ties():
    """C = 2 and G = 14: a cell whose two votes differ is a 1-1 tie, and with 14 meta-clusters the ids 10 .. 14 sort before 2 .. 9 as
    strings; then C = 4: 2-2 ties"""
    two = [wm_task(noisy_ensemble(300, 2, 14, 0.15, s), maxN=40) for s in TIE_SEEDS]
    four = [wm_task(noisy_ensemble(300, 4, 14, 0.15, 10 + s), maxN=40) for s in TIE_SEEDS[:2]]
    return tuple(two + four)


def string_order_cells(task, ref):
    """the cells whose winner is a tie that the string order of the ids decides otherwise than their numeric order would"""
    cid, _, _ = relabel(task["labels"])
    votes = ref["tf"][cid]
    n = 0
    for row in votes:
        ids, cnt = np.unique(row, return_counts=True)
        top = ids[cnt == cnt.max()]
        if top.size > 1 and min(top, key=str) != top.min():
            n += 1
    return n


@_cached
def list_fallback():
    """the single-winner fallback (R/wMetaC.R:148-161): every cell's first vote is one meta-cluster, so the runner-up is taken where there
    is one.  First: 60 cells, columns all 1, all 5, and 30 x 1 then 30 x 2 -> tf 1 1 1 2: the cells of the last column's second half have
    a runner-up, the others none (SHARP_WARN_NA_VOTE).  Second: three constant columns -> tf 1 1 2, every cell takes the runner-up."""
    one = np.stack([np.full(60, 1), np.full(60, 5), np.repeat([1, 2], 30)], 1)
    two = np.stack([np.full(40, 3), np.full(40, 7), np.full(40, 2)], 1)
    return (wm_task(one), wm_task(two))


WM_LISTS = {"mixed": list_mixed, "ragged": list_ragged, "lds_edge": list_lds_edge, "singletons": list_singletons, "vote_ties": list_vote_ties,
            "fallback": list_fallback}
_WM_REF = {}


def wm_reference(name):
    """(tasks, oracle results) of a list: computed once per process, shared by every test, read-only"""
    if name not in _WM_REF:
        tasks = WM_LISTS[name]()
        _WM_REF[name] = (tasks, tuple(oracle_wmetac(t) for t in tasks))
    return _WM_REF[name]


_WM_W = {}


def wm_exact_weights(name):
    """weights_exact of every task of a list, once per process"""
    if name not in _WM_W:
        _WM_W[name] = tuple(weights_exact(t["labels"]) for t in WM_LISTS[name]())
    return _WM_W[name]


def wm_list_margin_failures(name):
    tasks, refs = wm_reference(name)
    return [(name, i, why) for i, (t, r) in enumerate(zip(tasks, refs)) for why in wm_margin_failures(t, r)]


# ---- centroid means ----------------------------------------------------------------------------------------------------------------------

CM_SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 2, 3, 5, 12, 16, 17, 20, 24, 25, 30, 40, 44, 45)      # 24 clusters, 696 cells
CM_P = (1, 63, 64, 65, 130)


@_cached
def cm_uid(seed=2501):
    """first-appearance ids of 696 permuted cells: cluster t has CM_SIZES[t'] members for a permutation t' -- no cluster is contiguous"""
    lab = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(CM_SIZES)), CM_SIZES))
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    uid = rank[inv.ravel()].astype(np.int32)
    uid.setflags(write=False)
    return uid


@_cached
def cm_integer_E(p):
    """small integers: every partial sum is an integer below 2^53, so any order of addition is exact"""
    E = np.random.default_rng(2600 + p).integers(-1000, 1001, (sum(CM_SIZES), p)).astype(np.float64)
    E.setflags(write=False)
    return E


@_cached
def cm_mixed_E(p):
    """normal x 10^U(-3, 3), mixed signs"""
    rng = np.random.default_rng(2700 + p)
    E = rng.standard_normal((sum(CM_SIZES), p)) * 10.0 ** rng.uniform(-3, 3, (sum(CM_SIZES), p))
    E.setflags(write=False)
    return E


@_cached
def cm_mixed_ref(p):
    return cluster_means_ref(cm_mixed_E(p), cm_uid())


# ---- sMetaC --------------------------------------------------------------------------------------------------------------------------------

SM_P = 40
SM_OVERRIDE_SPREADS = (0.15, 0.3, 0.5)          # the oracle chooses k = 2 by more than 0.05 and overrides it to 3 or 4
SM_PLAIN_SPREAD = 1.0                         # the oracle chooses 6, no override


@_cached
def smetac_case(spread, seed=2809):
    """24 labelled clusters (CM_SIZES, cells permuted) around two far super-centres with three sub-centres each, four clusters per
    sub-centre, a cluster's own centre 0.4 off its sub-centre: up to a sub-centre spread of 0.5 the two super-centres are all the
    silhouette sees, at 1.0 the six sub-centres.  -> (labels, E)"""
    rng = np.random.default_rng(seed)
    uid = cm_uid()
    sup = rng.standard_normal((2, SM_P)) * 1.5
    sub = np.repeat(sup, 3, axis=0) + rng.standard_normal((6, SM_P)) * spread
    centre = sub[np.arange(len(CM_SIZES)) % 6] + rng.standard_normal((len(CM_SIZES), SM_P)) * 0.4
    E = centre[uid] + rng.standard_normal((uid.size, SM_P)) * 0.05
    labels = (uid * 7 + 3).astype(np.int32)                            # (any integers: only equality matters)
    E.setflags(write=False)
    return labels, E


def krange(ncells, nC, minN, maxN):
    """R/sMetaC.R:103-119: the candidate numbers of clusters by the number of cells"""
    if ncells < 1000000:
        baseN = min(max(ncells // 10000, 2), 10)
        if minN == 2 and min(maxN, nC) - baseN >= 3:
            minN = baseN
    else:
        maxN = max(maxN, ncells // 5000)
        minN = max(minN, ncells // 50000)
    return int(minN), int(maxN)


def smetac_hclust_task(means, ncells, minN=2, maxN=40, sil_thre=0.35):
    """the get_opt_hclust task inside sMetaC: the correlation of the centroids with a unit diagonal, the k range by ncells"""
    S = np.corrcoef(means)
    S = np.clip((S + S.T) / 2, -1.0, 1.0)
    np.fill_diagonal(S, 1.0)
    lo, hi = krange(ncells, means.shape[0], minN, maxN)
    t = make_hc_task(S, SIMILARITY, minN=lo, maxN=hi, sil_thre=sil_thre)
    t["tie"] = False
    return t


def logged(fn):
    """fn() with the oracle's decision log on -> (result, rows)"""
    o = _oracle()
    o.decision_log(True)
    try:
        res = fn()
        rows = o.last_decisions().copy()
    finally:
        o.decision_log(False)
    return res, rows


@_cached
def smetac_reference(spread):
    labels, E = smetac_case(spread)
    res, rows = logged(lambda: _oracle().sMetaC(labels, E))
    return res, rows


# ---- the k-range rules through the merge of centroid tables -----------------------------------------------------------------------------

KR_NCELLS = (9999, 10001, 29999, 30000, 99999, 100000, 999999, 1000000, 1500000)


@_cached
def krange_table(seed=2901):
    """60 centroid rows: 3 groups of 3 sub-groups of about 7 rows, and the cells behind every row (a few rows with fewer than 10)"""
    rng = np.random.default_rng(seed)
    p = 30
    top = rng.standard_normal((3, p)) * 4.0
    sub = np.repeat(top, 3, axis=0) + rng.standard_normal((9, p)) * 0.5
    rows = sub[np.arange(60) % 9] + rng.standard_normal((60, p)) * 0.3
    counts = rng.integers(10, 400, 60).astype(np.int64)
    counts[[4, 17, 33, 58]] = [3, 9, 1, 5]
    rows.setflags(write=False)
    counts.setflags(write=False)
    return rows, counts


@_cached
def krange_reference(ncells):
    M, cnt = krange_table()
    return logged(lambda: _oracle().unlimited_merge(M, cnt, ncells))
