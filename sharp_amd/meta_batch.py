"""The test entries of the meta-clustering stage (include/sharp_hip.h): sharp_wMetaC_batch, a whole batch of wMetaC tasks through one
wmetac_batch call, and sharp_cluster_means / sharp_ensemble_mean, one call each of the centroid means and of the ensemble mean on host
arrays.  make_task / base_clusters / pack_tasks / capacities / unpack_results are plain numpy and need no library:
tests/test_meta_cpu.py checks the concatenation and the offsets on their own."""
import numpy as np

from ._lib import check, f64, i32, i64, lib, ensure_init
from .api import HMETHODS
from .hclust_batch import INT_SENTINEL, NAN_SENTINEL_BITS, is_sentinel  # noqa: F401  (the entries share the sentinels)

OUTPUTS = ("rc", "allC", "ncl", "finalC", "w1", "S", "tf", "x0")            # the order of cap[8]
DOUBLES = ("w1", "S", "x0")
WARN_RANGE, WARN_NA_VOTE = 16, 32
MAX_BASE_CLUSTERS = 65535
PAD = 5                                                                    # values of room behind what a call is expected to write


def make_task(labels, hmethod="ward.D", enN_cluster=0, minN=2, maxN=40, sil_thre=0.35, height_Ntimes=2.0):
    """one wMetaC task: labels (N, C) integers, equal within a column <=> same base cluster"""
    lab = np.asarray(labels)
    if lab.ndim != 2 or lab.dtype.kind not in "iu":
        raise TypeError("labels must be an N x C matrix of integers")
    return dict(labels=np.asfortranarray(lab, dtype=np.int32), hmethod=hmethod, enN_cluster=int(enN_cluster), minN=int(minN), maxN=int(maxN),
                sil_thre=float(sil_thre), height_Ntimes=float(height_Ntimes))


def base_clusters(task):
    """allC: the distinct labels of every column, summed"""
    lab = task["labels"]
    return int(sum(np.unique(lab[:, c]).size for c in range(lab.shape[1])))


def pack_tasks(tasks):
    """the entry's parallel input arrays; the label matrices one after the other, column-major"""
    i = lambda key: np.array([t[key] for t in tasks], np.int32)      # noqa: E731
    d = lambda key: np.array([t[key] for t in tasks], np.float64)    # noqa: E731
    hm = np.array([t["hmethod"] if isinstance(t["hmethod"], (int, np.integer)) else HMETHODS[t["hmethod"]] for t in tasks], np.int32)
    return dict(N=np.array([t["labels"].shape[0] for t in tasks], np.int32), C=np.array([t["labels"].shape[1] for t in tasks], np.int32),
                hmethod=hm, enN_cluster=i("enN_cluster"), minN=i("minN"), maxN=i("maxN"), sil_thre=d("sil_thre"),
                height_Ntimes=d("height_Ntimes"),
                labels=np.concatenate([t["labels"].ravel(order="F") for t in tasks] + [np.zeros(0, np.int32)]).astype(np.int32))


def capacities(tasks, pad=PAD):
    """room for everything a batch can write, and `pad` values more behind it: the meta-clusters of a task number at most enN_cluster, or
    min(maxN, allC - 1); a task with more base clusters than the driver takes gets no room for S, tf and x0 (it is refused)"""
    N = [t["labels"].shape[0] for t in tasks]
    A = [base_clusters(t) for t in tasks]
    A = [a if a <= MAX_BASE_CLUSTERS else 0 for a in A]
    k = [t["enN_cluster"] if t["enN_cluster"] > 0 else max(1, min(t["maxN"], a - 1)) for t, a in zip(tasks, A)]
    cap = dict(rc=len(tasks), allC=len(tasks), ncl=len(tasks), finalC=sum(N), w1=sum(N), S=sum(a * a for a in A), tf=sum(A),
               x0=sum(n * kk for n, kk, a in zip(N, k, A) if a))
    return {key: int(v) + pad for key, v in cap.items()}


def alloc_outputs(cap):
    """zero-filled: the entry writes the sentinels itself"""
    return {key: np.zeros(cap[key], np.float64 if key in DOUBLES else np.int32) for key in OUTPUTS}


def written(out, N):
    """how many values of every output a finished batch wrote, from its own allC and ncl"""
    count = len(N)
    allC, ncl = out["allC"][:count].astype(np.int64), out["ncl"][:count].astype(np.int64)
    N = np.asarray(N, np.int64)
    return dict(rc=count, allC=count, ncl=count, finalC=int(N.sum()), w1=int(N.sum()), S=int((allC * allC).sum()), tf=int(allC.sum()),
                x0=int((N * ncl).sum()))


def unpack_results(out, N):
    """one dict per task: rc, allC, ncl, finalC (N), w1 (N), S (allC, allC), tf (allC), x0 (N, ncl)"""
    count = len(N)
    N = np.asarray(N, np.int64)
    allC, ncl = out["allC"][:count].astype(np.int64), out["ncl"][:count].astype(np.int64)
    cum = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)   # noqa: E731
    oN, oS, oT, oX = cum(N), cum(allC * allC), cum(allC), cum(N * ncl)
    res = []
    for t in range(count):
        a, k, n = int(allC[t]), int(ncl[t]), int(N[t])
        res.append(dict(rc=int(out["rc"][t]), allC=a, ncl=k, finalC=out["finalC"][oN[t]: oN[t + 1]].copy(), w1=out["w1"][oN[t]: oN[t + 1]].copy(),
                        S=out["S"][oS[t]: oS[t + 1]].reshape(a, a).copy(), tf=out["tf"][oT[t]: oT[t + 1]].copy(),
                        x0=out["x0"][oX[t]: oX[t + 1]].reshape(k, n).T.copy()))
    return res


def wmetac_batch(tasks, cap=None, null_labels=False, raw=False):
    """ONE wmetac_batch call over `tasks` (make_task), with x0 and the intermediates.  cap: capacities to state instead of
    capacities(tasks) (a dict; missing keys keep theirs).  raw: also return the output arrays as the entry left them.  A refusal raises
    SharpError with the arrays, all sentinel, in its `outputs` attribute."""
    ensure_init()
    a = pack_tasks(tasks)
    caps = capacities(tasks)
    caps.update(cap or {})
    out = alloc_outputs(caps)
    capv = np.array([caps[key] for key in OUTPUTS], np.int64)
    try:
        check(lib().sharp_wMetaC_batch(len(tasks), i32(a["N"]), i32(a["C"]), i32(a["hmethod"]), i32(a["enN_cluster"]), i32(a["minN"]),
                                       i32(a["maxN"]), f64(a["sil_thre"]), f64(a["height_Ntimes"]), None if null_labels else i32(a["labels"]),
                                       i64(capv), *[(f64 if key in DOUBLES else i32)(out[key]) for key in OUTPUTS]))
    except Exception as e:
        e.outputs = out
        raise
    res = unpack_results(out, a["N"])
    return (res, out) if raw else res


def cluster_means(E, uid, nC=None, ld=None, pad=PAD):
    """sharp_cluster_means: the mean row of every cluster of E (n, p); the rows are laid out with leading dimension ld (default p), the
    values between the rows NaN.  Returns the whole output buffer: nC * p means and `pad` values behind them."""
    ensure_init()
    E = np.ascontiguousarray(E, np.float64)
    n, p = E.shape
    ld = p if ld is None else int(ld)
    uid = np.ascontiguousarray(uid, np.int32)
    nC = int(uid.max()) + 1 if nC is None else int(nC)
    host = np.full(n * ld, np.nan)
    host.reshape(n, ld)[:, :p] = E
    out = np.zeros(nC * p + pad)
    check(lib().sharp_cluster_means(f64(host), ld, n, p, i32(uid), nC, f64(out), out.size))
    return out


def ensemble_mean(E, K, p, ldE=None, pad=PAD):
    """sharp_ensemble_mean of E (n, K * p), laid out with leading dimension ldE (default K * p), NaN between the rows.  Returns the whole
    output buffer: n * p values and `pad` behind them."""
    ensure_init()
    E = np.ascontiguousarray(E, np.float64)
    n = E.shape[0]
    assert E.shape[1] == K * p
    ldE = K * p if ldE is None else int(ldE)
    host = np.full(n * ldE, np.nan)
    host.reshape(n, ldE)[:, : K * p] = E
    out = np.zeros(n * p + pad)
    check(lib().sharp_ensemble_mean(f64(host), ldE, n, p, K, f64(out), out.size))
    return out
