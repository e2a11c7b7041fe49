"""The test entry for a whole batch of get_opt_hclust tasks (sharp_get_opt_hclust_batch, include/sharp_hip.h) and the plan record of
what the batch driver did with it (sharp_hclust_batch_plan).  pack_tasks / output_layout / alloc_outputs / unpack_results are plain
numpy and need no library: tests/test_hclust_batch_cpu.py checks the concatenation and the offsets on their own."""
import ctypes as C

import numpy as np

from ._lib import check, f64, i32, lib, ensure_init
from .api import HMETHODS

PLAN_COLUMNS = ("i0", "i1", "slot", "pipe", "split", "NS", "ml", "max_n", "max_kpad", "seq_deferred", "form", "gs", "nested", "max_nk", "wpt",
                "finish_at")
FORM_NONE, FORM_SPLIT, FORM_1024, FORM_512 = 0, 1, 2, 3
INT_SENTINEL = np.iinfo(np.int32).min
NAN_SENTINEL_BITS = 0x7FF8C0DE5EED0001
FEATURES, SIMILARITY = 0, 1


def make_task(mat, kind=FEATURES, hmethod="ward.D", N_cluster=0, minN=2, maxN=40, sil_thre=0.35, height_Ntimes=2.0):
    return dict(mat=np.ascontiguousarray(mat, np.float64), kind=int(kind), hmethod=hmethod, N_cluster=int(N_cluster), minN=int(minN),
                maxN=int(maxN), sil_thre=float(sil_thre), height_Ntimes=float(height_Ntimes))


def nk_of(task):
    """candidate levels of a task, as the entry sizes its outputs"""
    n = task["mat"].shape[0]
    return 1 if task["N_cluster"] > 0 else max(1, min(task["maxN"], n - 1) - task["minN"] + 1)


def pack_tasks(tasks):
    """the entry's parallel input arrays; the matrices one after the other, row-major"""
    i = lambda key: np.array([t[key] for t in tasks], np.int32)      # noqa: E731
    d = lambda key: np.array([t[key] for t in tasks], np.float64)    # noqa: E731
    hm = np.array([t["hmethod"] if isinstance(t["hmethod"], (int, np.integer)) else HMETHODS[t["hmethod"]] for t in tasks], np.int32)
    return dict(n=np.array([t["mat"].shape[0] for t in tasks], np.int32), p=np.array([t["mat"].shape[1] for t in tasks], np.int32),
                kind=i("kind"), hmethod=hm, N_cluster=i("N_cluster"), minN=i("minN"), maxN=i("maxN"), sil_thre=d("sil_thre"),
                height_Ntimes=d("height_Ntimes"), mats=np.concatenate([t["mat"].ravel() for t in tasks]))


def output_layout(n, nk):
    """offsets (count + 1 each) of every task in f, v, msil / CHind and height"""
    n = np.asarray(n, np.int64)
    nk = np.asarray(nk, np.int64)
    cum = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)   # noqa: E731
    return dict(f=cum(n), v=cum(n * nk), k=cum(nk), h=cum(n - 1))


def alloc_outputs(n, nk, want_v, sets=1):
    """the entry's output arrays for `sets` sets of results (two with nested), zero-filled: the entry writes the sentinels itself"""
    lay = output_layout(n, nk)
    count = len(n)
    out = dict(f=np.zeros(sets * lay["f"][-1], np.int32), v=np.zeros(sets * lay["v"][-1], np.int32) if want_v else None,
               msil=np.zeros(sets * lay["k"][-1]), CHind=np.zeros(sets * lay["k"][-1]), height=np.zeros(sets * lay["h"][-1]))
    for key in ("optN", "nk", "branch", "rc", "sequential"):
        out[key] = np.zeros(sets * count, np.int32)
    return out


def unpack_results(out, n, nk, want_v, which=0):
    """set `which` of the output arrays as one dict per task; v as (n, nk), one column per level, like api.get_opt_hclust"""
    lay = output_layout(n, nk)
    count = len(n)
    res = []
    for t in range(count):
        part = lambda a, o: a[which * o[-1] + o[t]: which * o[-1] + o[t + 1]].copy()   # noqa: E731
        r = dict(f=part(out["f"], lay["f"]), msil=part(out["msil"], lay["k"]), CHind=part(out["CHind"], lay["k"]),
                 height=part(out["height"], lay["h"]))
        r["v"] = part(out["v"], lay["v"]).reshape(int(nk[t]), int(n[t])).T.copy() if want_v else None
        for key in ("optN", "nk", "branch", "rc", "sequential"):
            r[key] = int(out[key][which * count + t])
        res.append(r)
    return res


def get_opt_hclust_batch(tasks, want_v=True, nested=False):
    """ONE get_opt_hclust_batch call over `tasks` (make_task).  Returns the per-task results, and with nested a second list: the same
    tasks run again from the batch's progress callback (sentinels where a task was never reported, see the header)."""
    ensure_init()
    a = pack_tasks(tasks)
    nk = np.array([nk_of(t) for t in tasks], np.int64)
    sets = 2 if nested else 1
    out = alloc_outputs(a["n"], nk, want_v, sets)
    check(lib().sharp_get_opt_hclust_batch(len(tasks), i32(a["n"]), i32(a["p"]), i32(a["kind"]), i32(a["hmethod"]), i32(a["N_cluster"]),
                                           i32(a["minN"]), i32(a["maxN"]), f64(a["sil_thre"]), f64(a["height_Ntimes"]), f64(a["mats"]),
                                           int(want_v), int(nested), i32(out["f"]), i32(out["v"]), f64(out["msil"]), f64(out["CHind"]),
                                           f64(out["height"]), i32(out["optN"]), i32(out["nk"]), i32(out["branch"]), i32(out["rc"]),
                                           i32(out["sequential"])))
    first = unpack_results(out, a["n"], nk, want_v, 0)
    return (first, unpack_results(out, a["n"], nk, want_v, 1)) if nested else first


def batch_plan():
    """sharp_hclust_batch_plan: one dict (PLAN_COLUMNS) per chunk of the calling context's last batch"""
    ensure_init()
    n = C.c_int()
    check(lib().sharp_hclust_batch_plan(None, 0, C.byref(n)))
    rows = np.zeros((max(n.value, 1), len(PLAN_COLUMNS)), np.int32)
    check(lib().sharp_hclust_batch_plan(i32(rows), n.value, C.byref(n)))
    return [dict(zip(PLAN_COLUMNS, map(int, r))) for r in rows[: n.value]]


def is_sentinel(a):
    """where an output still holds what the entry filled it with"""
    a = np.asarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64) == np.uint64(NAN_SENTINEL_BITS)
    return a == INT_SENTINEL
