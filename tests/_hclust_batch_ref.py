"""CPU side of the get_opt_hclust batch tests (tests/test_hclust_batch_gpu.py, tests/test_hclust_batch_cpu.py): the task lists, their
expected results from the oracle (one task at a time, computed once per process and never changed), and check_margins, which decides
from the oracle's numbers alone whether a task's labels and level choice can be demanded EXACTLY of another implementation.

Every list is built from fixed seeds, and every task of every list passes check_margins: test_hclust_batch_cpu.py asserts that here,
the GPU tests assert it again.  No task is ever left out of a comparison.

Thresholds of the batch driver that the lists are sized by, from sharp_amd/csrc (stated here once; the GPU tests assert the plan record,
so a list that no longer reaches its regime fails there):
  kHcSplitMaxTasks = 136, kHcSplitMinObs = 1000   hclust.hip: a chunk of at most 136 tasks with max_n >= 1000 takes the round-per-launch form
  T >= 194                                        hclust.hip, setup_chunk: two ranges
  HR_MAXN = 4096                                  hclust_task.hpp: above, the bulk-synchronous kernel keeps its state in global memory
  nld <= 2048                                     hclust.hip, setup_chunk: feature tasks whose distance GEMM leaves row minima
  64 finest clusters (kpad <= 64)                 hclust_stats.hip: stats_lane_kernel, above stats_kernel
  kMlMinLevels = 256 (SHARP_ML_MIN_LEVELS)        hclust.hip: more candidate levels in a chunk -> ml_*_kernel
"""
import functools

import numpy as np

from sharp_amd.hclust_batch import FEATURES, SIMILARITY, make_task

K_SPLIT_MAX_TASKS = 136
K_SPLIT_MIN_OBS = 1000
K_TWO_RANGES_TASKS = 194
HR_MAXN = 4096
NN_PARTS_MAX_NLD = 2048
LANE_MAX_KPAD = 64
NUM_CU = 256                       # MI355X

REDUCIBLE = ("ward.D", "ward.D2", "average", "complete", "single", "mcquitty")
NOT_REDUCIBLE = ("centroid", "median")


def _oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


# ---- generators -----------------------------------------------------------------------------------------------------------------------

def gaussian_mixture(n, p, G, seed, spread=2.0):
    """planted Gaussian mixture, as tests/test_hclust_gpu.py builds them: unit noise around G centres"""
    rng = np.random.default_rng(seed)
    G = max(1, min(G, n))
    return rng.standard_normal((n, p)) + rng.standard_normal((G, p))[rng.integers(0, G, n)] * spread


def feature_task(n, p, G, seed, spread=2.0, **kw):
    t = make_task(gaussian_mixture(n, p, G, seed, spread), FEATURES, **kw)
    t["tie"] = False
    return t


def similarity_task(n, p, G, seed, **kw):
    """np.corrcoef of a mixture, symmetrised, unit diagonal"""
    S = np.corrcoef(gaussian_mixture(n, p, G, seed))
    np.fill_diagonal(S, 1.0)
    t = make_task((S + S.T) / 2, SIMILARITY, **kw)
    t["tie"] = False
    return t


def wmetac_similarity_task(N, cols, G, seed, flip=0.05, **kw):
    """oracle.wMetaC(...)["S"] of `cols` noisy copies of one partition: the wMetaC / sMetaC call shape (exact ones off the diagonal)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, G + 1, N)
    parts = [base.copy() for _ in range(cols)]
    for c in parts[1:]:
        f = rng.random(N) < flip
        c[f] = rng.integers(1, G + 1, f.sum())
    t = make_task(_oracle().wMetaC(np.stack(parts, 1))["S"], SIMILARITY, **kw)
    t["tie"] = False
    return t


def saturated_similarity_task(N, G, seed, **kw):
    """wMetaC of identical partitions: silhouettes exactly 1 at several levels (R/get_opt_hclust.R:162-168 takes the middle arg-max)"""
    base = np.random.default_rng(seed).integers(1, G + 1, N)
    t = make_task(_oracle().wMetaC(np.stack([base, base % G + 1, base], 1))["S"], SIMILARITY, **kw)
    t["tie"] = True                    # (equal similarities: exact ties in the distances as well)
    t["saturated"] = True
    return t


def weak_task(seed, **kw):
    """weak structure, as test_get_opt_hclust_ch_and_height_branches builds it: every median silhouette below sil.thre, so CH decides, or
    (height_Ntimes close to 1) the height rule"""
    Y = np.random.default_rng(seed).normal(size=(150, 40))
    Y[:50, :5] += 0.8
    t = make_task(Y, FEATURES, **kw)
    t["tie"] = False
    return t


def tie_task(n, p, G, seed, dup, **kw):
    """`dup` rows duplicated (the last dup rows repeat the first dup): exact ties, which the bulk-synchronous kernel abandons to the
    sequential one.  n >= 2 maxN, so that no candidate level cuts through the duplicates (the rule of
    test_lane_program_statistics_equal_the_per_cell_walk)."""
    E = gaussian_mixture(n, p, G, seed)
    E[n - dup:] = E[:dup]
    t = make_task(E, FEATURES, **kw)
    assert n >= 2 * t["maxN"] and 2 * dup <= n
    t["tie"] = True
    return t


# ---- the oracle's result of a task, and whether it can be demanded exactly ---------------------------------------------------------------

def oracle_result(task):
    o = _oracle()
    r = o.get_opt_hclust(task["mat"], hmethod=task["hmethod"], N_cluster=task["N_cluster"], minN=task["minN"], maxN=task["maxN"],
                         sil_thre=task["sil_thre"], height_Ntimes=task["height_Ntimes"])
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def expected_sequential(task):
    """1 exactly for tie tasks and centroid / median"""
    return int(task["tie"] or task["hmethod"] in NOT_REDUCIBLE)


def check_margins(task, ref):
    """[] if labels, level and branch of `task` can be demanded exactly given the comparison tolerances (msil 1e-10 absolute, CH 1e-8 and
    heights 1e-9 relative), else the reasons.  From the oracle's result `ref` alone.
      - the deciding maximum (msil, or CH in the CH / height branches) beats the largest value strictly below it by more than 1e-8
        relative (values EQUAL to it are exact ties, which the rule resolves by position); max(msil) is more than 1e-8 from sil.thre;
        where the height rule was consulted, each of its comparisons has more than 1e-8 relative to spare;
      - the heights of the merges that separate the levels kmin - 1 .. kmax differ from their neighbours by more than 1e-9 relative
        (aside: pairs of heights within the comparison's absolute tolerance of zero, i.e. merges of duplicated rows, and in a tie task
        heights that are exactly equal)."""
    why = []
    n = task["mat"].shape[0]
    h = ref["height"]
    if task["N_cluster"] > 0:
        kmin = kmax = task["N_cluster"]
    else:
        kmin, kmax = task["minN"], min(task["maxN"], n - 1)
    # level k = the first n - k merges: steps n - kmax - 1 .. n - kmin + 2 (1-based) must be strictly ordered
    lo, hi = max(1, n - kmax - 1), min(n - 1, n - kmin + 2)
    for s in range(lo, hi):
        a, b = h[s - 1], h[s]
        if (abs(a) <= 1e-12 and abs(b) <= 1e-12) or (task["tie"] and a == b):     # (exactly equal: R's order, which the sequential kernel keeps)
            continue
        if not abs(b - a) > 1e-9 * max(abs(a), abs(b)):
            why.append(f"heights of merges {s} and {s + 1} too close: {a!r} {b!r}")
    if task["N_cluster"] > 0:
        return why
    msil, ch = ref["msil"], ref["CHind"]
    mx = msil.max()
    if not abs(mx - task["sil_thre"]) > 1e-8:
        why.append(f"max msil {mx!r} at the threshold")

    def runner_up(val, what):
        best = val.max()
        below = val[val < best]
        if below.size and not best - below.max() > 1e-8 * abs(best):
            why.append(f"{what}: best {best!r} runner-up {below.max()!r}")

    if ref["branch"] == 0:
        runner_up(msil, "msil")
    else:
        if not np.all(np.isfinite(ch)):
            why.append("CH decides and is not finite")
        runner_up(ch, "CH")
        if int(np.argmax(ch)) == 0:                    # the height rule (R/get_opt_hclust.R:196-210)
            nh = n - 1
            tmp = h[max(0, nh - 10):]
            hit = None
            for i in range(len(tmp) - 1):
                dif, den = tmp[i + 1] - tmp[i], (task["height_Ntimes"] - 1) * tmp[i]
                if not abs(dif - den) > 1e-8 * max(abs(dif), abs(den)):
                    why.append(f"height rule step {i}: gap {dif!r} against {den!r}")
                if dif > den:
                    hit = i
                    break
            if hit is not None:
                opth = (tmp[hit] + tmp[hit + 1]) / 2
                if not np.all(np.abs(h - opth) > 1e-9 * opth):
                    why.append("height rule: a height at the cut")
    return why


# ---- the task lists of the GPU tests (each built once per process) --------------------------------------------------------------------

def _cached(fn):
    return functools.lru_cache(maxsize=None)(fn)


@_cached
def list_mixed_sizes():
    """1: one task of 1000 observations puts the chunk on the round-per-launch path; the small ones finish within the first rounds"""
    return tuple(feature_task(n, 24, 5, 1100 + n, maxN=10) for n in (1000, 3, 40, 127, 128, 129, 300, 999))


@_cached
def list_linkages():
    """2: every linkage once, n around 150"""
    hms = REDUCIBLE + NOT_REDUCIBLE
    return tuple(feature_task(141 + 3 * i, 30, 4, 1200 + i, hmethod=hm, maxN=12) for i, hm in enumerate(hms))


@_cached
def list_interleaved():
    """3: F, S, S, F, S with different n, and a saturated similarity"""
    return (feature_task(200, 40, 5, 1301, maxN=20), similarity_task(97, 30, 3, 1302, maxN=20),
            wmetac_similarity_task(400, 5, 6, 1303, maxN=20), feature_task(130, 16, 4, 1304, maxN=20),
            similarity_task(64, 20, 3, 1305, maxN=20), saturated_similarity_task(300, 6, 1306, maxN=20))


@_cached
def list_nn_parts():
    """4: row-minimum parts for the second and fourth task only"""
    return (feature_task(2049, 20, 6, 1401, maxN=10), feature_task(300, 20, 4, 1402, maxN=10), similarity_task(200, 30, 4, 1403, maxN=10),
            feature_task(2048, 20, 6, 1404, maxN=10))


@_cached
def list_kpad():
    """5a: kpad 16 .. 64, and last a task with 70 finest clusters"""
    return tuple(feature_task(150 + 7 * i, 40, 6, 1500 + i, maxN=m) for i, m in enumerate((15, 16, 17, 40, 64, 70)))


@_cached
def list_many_levels():
    """5b: nk = 30, 3 and 1 (N_cluster given), features and a similarity"""
    return (feature_task(120, 30, 5, 1511, minN=3, maxN=32), feature_task(90, 30, 3, 1512, minN=2, maxN=4),
            feature_task(100, 30, 4, 1513, N_cluster=5), similarity_task(80, 30, 3, 1514, minN=2, maxN=4))


@_cached
def list_given_and_short():
    """5c: N_cluster given beside ranges, n - 1 < maxN, and two tasks that the CH rule and the height rule decide"""
    return (feature_task(110, 30, 4, 1521, N_cluster=3), feature_task(140, 30, 5, 1522, maxN=40), feature_task(12, 30, 2, 1523, maxN=40),
            similarity_task(75, 30, 3, 1524, N_cluster=4), feature_task(60, 30, 3, 1525, minN=3, maxN=9), weak_task(7, maxN=40),
            weak_task(8, maxN=40, height_Ntimes=1.05))


@_cached
def list_fallback():
    """6 / 10: five tasks of about 300 observations, tasks 1 and 3 with duplicated rows"""
    return (feature_task(300, 30, 5, 1601, maxN=20), tie_task(290, 30, 4, 1602, 40, maxN=20), feature_task(310, 30, 6, 1603, maxN=20),
            tie_task(305, 30, 5, 1604, 25, maxN=20), feature_task(295, 30, 4, 1605, maxN=20))


@_cached
def _pool():
    """20 distinct data sets of 24 .. 60 observations, and 4 with duplicated rows (n >= 2 maxN = 16)"""
    plain = tuple(gaussian_mixture(24 + (11 * i) % 37, 16, 3 + i % 3, 1700 + i) for i in range(20))
    ties = []
    for i in range(4):
        E = gaussian_mixture(30 + 9 * i, 16, 3, 1750 + i)
        E[-6:] = E[:6]
        ties.append(E)
    return plain, tuple(ties)


def _cycled(count, tie_at):
    """`count` tasks of the pool's data sets in rotation with k-ranges in rotation (maxN 8, 7, 6; minN 2, 3), tie tasks at `tie_at`"""
    plain, ties = _pool()
    out = []
    for t in range(count):
        if t in tie_at:
            task = make_task(ties[sorted(tie_at).index(t) % len(ties)], FEATURES, maxN=8)
            task["tie"] = True
        else:
            task = make_task(plain[t % len(plain)], FEATURES, minN=2 + (t // 20) % 2, maxN=8 - (t // 40) % 3)
            task["tie"] = False
        out.append(task)
    return tuple(out)


@_cached
def list_two_ranges():
    """7: 194 ragged tasks, ties on both sides of the range boundary and at both ends, and one (150) whose place in the other range (53)
    holds a task without ties"""
    return _cycled(194, (0, 96, 97, 150, 193))


@_cached
def list_three_ranges():
    """7: seven tasks for SHARP_HC_RANGES=3 (ranges [0, 2), [2, 4), [4, 7)): the middle range holds a tie task"""
    return _cycled(7, (3,))


@_cached
def list_many(count):
    """8: more tasks than CUs, a handful of tie tasks spread over the chunks"""
    return _cycled(count, tuple(sorted({1, count // 4, count // 2, count // 2 + 1, count - 130, count - 1})))


@_cached
def list_global_state():
    """9: one task beyond HR_MAXN makes the whole chunk keep its agglomeration state in global memory"""
    rng = np.random.default_rng(5)
    big = rng.standard_normal((4100, 40)) + np.repeat(rng.standard_normal((10, 40)) * 3.0, 410, axis=0)
    t = make_task(big, FEATURES, maxN=12)
    t["tie"] = False
    return (t, feature_task(50, 40, 3, 1902, maxN=12), feature_task(1000, 40, 8, 1903, maxN=12))


ALL_LISTS = {
    "mixed_sizes": list_mixed_sizes, "linkages": list_linkages, "interleaved": list_interleaved, "nn_parts": list_nn_parts,
    "kpad": list_kpad, "many_levels": list_many_levels, "given_and_short": list_given_and_short, "fallback": list_fallback,
    "two_ranges": list_two_ranges, "three_ranges": list_three_ranges, "many_257": lambda: list_many(257),
    "many_513": lambda: list_many(513), "many_300": lambda: list_many(300), "global_state": list_global_state,
}

_REF = {}


def reference(name):
    """(tasks, oracle results) of a list; the results are computed once per distinct task (by the identity of its matrix and its
    parameters), shared by every test and read-only"""
    tasks = ALL_LISTS[name]()
    refs = []
    for t in tasks:
        key = (id(t["mat"]), t["kind"], t["hmethod"], t["N_cluster"], t["minN"], t["maxN"], t["sil_thre"], t["height_Ntimes"])
        if key not in _REF:
            _REF[key] = (t["mat"], oracle_result(t))        # (the matrix is kept alive: its id stays its own)
        refs.append(_REF[key][1])
    return tasks, refs


def margin_failures(name):
    tasks, refs = reference(name)
    return [(name, i, why) for i, (t, r) in enumerate(zip(tasks, refs)) for why in check_margins(t, r)]
