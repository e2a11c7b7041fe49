"""sharp_C_scrublet_csc called the way R's .C() calls a native routine (every argument a pointer into a caller-owned vector, the status
last): the bits of the Python call.  This is the call r/sharp_hip.R::sharp_scrublet makes."""
import ctypes as C

import numpy as np
import pytest

import _doublets_ref as R
import _expr_pca_ref as ref
from sharp_amd import doublets  # noqa: F401  (without the feature every test here fails at import)

pytestmark = pytest.mark.gpu


def I(*v):
    return np.array(v, np.int32)


def D(*v):
    return np.array(v, np.float64)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def last_error(lib):
    buf = C.create_string_buffer(b" " * 2047)
    ptr = (C.c_char_p * 1)(C.addressof(buf))
    lib.sharp_C_last_error(ptr, P(I(2048)))
    return buf.value.decode()


def cat(blocks):
    return (np.concatenate([np.asarray(b.indptr, np.int32) for b in blocks]), np.concatenate([np.asarray(b.indices, np.int32) for b in blocks] + [I()]),
            np.concatenate([np.asarray(b.data, np.float64) for b in blocks] + [D()]), D(*[b.shape[1] for b in blocks]))


def dotc_scrublet(sa, blocks, m, n, k, top, genes=None, fit=None, threshold=np.nan, ratio=2.0, seed=0, slab=0):
    n_sim = R.plan(n, ratio)[0]
    pc, ic, xc, ncb = cat(blocks)
    g = I(0) if genes is None else np.asarray(genes, np.int32)
    f = [D(0)] * 4 if fit is None else [np.ascontiguousarray(fit[key], np.float64) for key in ("scores", "loadings", "center", "scale")]
    out = {"sc": np.zeros(n), "ss": np.zeros(n_sim), "pred": np.zeros(n, np.int32), "thr": D(0), "found": I(-1), "rates": np.zeros(3), "nn": I(0),
           "ka": I(0), "par": np.zeros(2 * n_sim, np.int32), "genes": np.zeros(max(top, g.size), np.int32), "ng": I(-1),
           "counts": np.zeros(n + n_sim, np.int32), "sim": np.zeros(n_sim * k), "st": I(-1)}
    args = [pc, ic, xc, I(len(blocks)), ncb, I(m), D(ratio), D(0.1), I(0), I(k), I(top), g, I(0 if genes is None else g.size), I(fit is not None)] + f + [
        D(1e4), I(1), I(1), D(threshold), I(0), I(0), D(0, 0, 0, 0, 0), D(seed), I(slab), out["sc"], out["ss"], out["pred"], out["thr"], out["found"],
        out["rates"], out["nn"], out["ka"], out["par"], out["genes"], out["ng"], out["counts"], I(1), out["sim"], out["st"]]
    sa.lib().sharp_C_scrublet_csc(*[P(a) for a in args])
    return out


def test_dotc_scrublet(sa):
    n, m, k, top = 400, 400, 10, 150
    blocks = ref.ragged(ref.planted(n, m, 4)[0], [130, 131])
    want = sa.scrublet(blocks, n_prin_comps=k, n_top_genes=top, ret_sim=True)
    got = dotc_scrublet(sa, blocks, m, n, k, top, slab=50)
    assert got["st"][0] == 0, last_error(sa.lib())
    assert got["sc"].tobytes() == want["doublet_scores"].tobytes() and got["ss"].tobytes() == want["doublet_scores_sim"].tobytes()
    assert np.array_equal(got["counts"], want["neighbor_counts"]) and np.array_equal(got["par"].reshape(-1, 2), want["parents"])
    assert got["ng"][0] == want["genes"].size and np.array_equal(got["genes"][:got["ng"][0]], want["genes"])
    assert (got["nn"][0], got["ka"][0]) == (want["n_neighbors"], want["k_adj"])
    assert got["sim"].tobytes() == want["sim_pca"].tobytes()
    assert bool(got["found"][0]) == want["threshold_found"]
    if want["threshold_found"]:
        assert got["thr"][0] == want["threshold"] and np.array_equal(got["pred"].astype(bool), want["predicted_doublets"])
        assert got["rates"].tolist() == [want["detected_doublet_rate"], want["detectable_doublet_fraction"], want["overall_doublet_rate"]]
    else:
        assert np.isnan(got["thr"][0])
    # the caller's fit and a given threshold
    fit = sa.expression_pca(blocks, k, scale=True, genes=want["genes"])
    got = dotc_scrublet(sa, blocks, m, n, k, top, genes=want["genes"], fit=fit, threshold=0.2)
    assert got["st"][0] == 0, last_error(sa.lib())
    assert got["sc"].tobytes() == want["doublet_scores"].tobytes() and got["thr"][0] == 0.2 and got["found"][0] == 0
    assert np.array_equal(got["pred"].astype(bool), want["doublet_scores"] > 0.2)
    # refusals reach R's error() with the library's names
    got = dotc_scrublet(sa, blocks, m, n, k, top, ratio=0.001)
    assert got["st"][0] != 0 and "scrublet: sim_doublet_ratio gives fewer than 1 simulated doublet" in last_error(sa.lib())
