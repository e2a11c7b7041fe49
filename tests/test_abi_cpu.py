"""The Python binding's one statement of the C ABI (sharp_amd/_abi.py) against include/sharp_hip.h, and the marshalling of the package's
entry points: what they pass reaches the library as the header declares it, and what the library must not be handed is refused first.
No GPU is needed: without a device every compute entry fails with the library's own message, after its arguments were converted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SCALARS = {"int": "i", "unsigned": "u", "long long": "l", "double": "d"}
_RETURNS = {"int": "i", "void": "v", "const char *": "s"}


def _header_signatures():
    """{name: "<return>:<argument kinds>"} in _abi's notation, parsed from the header"""
    src = open(os.path.join(ROOT, "include", "sharp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    out = {}
    for ret, name, args in re.findall(r"\b(const\s+char\s*\*|int|void)\s*(sharp_\w+)\s*\(([^)]*)\)\s*;", src):
        kinds = ""
        for a in ([] if args.strip() == "void" else args.split(",")):
            a = " ".join(a.split())
            kinds += "p" if "*" in a else _SCALARS[re.sub(r"\s*\w+$", "", a)]       # (a KeyError: a kind the binding does not know)
        assert name not in out, f"{name} is declared twice"
        out[name] = _RETURNS[" ".join(ret.replace("*", " * ").split())] + ":" + kinds
    return out


@pytest.fixture(scope="module")
def sharp():
    import __graft_entry__ as g

    import sharp_amd

    if not os.path.exists(sharp_amd.so_path()):
        g.build()
    return sharp_amd


def test_table_equals_header():
    from sharp_amd import _abi

    header = _header_signatures()
    assert len(header) >= 121 and len(_abi.SIGNATURES) >= 121
    assert sorted(set(header) - set(_abi.SIGNATURES)) == [], "declared in include/sharp_hip.h, missing from sharp_amd/_abi.py"
    assert sorted(set(_abi.SIGNATURES) - set(header)) == [], "in sharp_amd/_abi.py, not declared in include/sharp_hip.h"
    wrong = {n: (_abi.SIGNATURES[n], header[n]) for n in header if _abi.SIGNATURES[n] != header[n]}
    assert not wrong, f"(table, header) differ: {wrong}"
    assert {s.split(":")[0] for s in header.values()} == {"i", "v", "s"}
    assert set("".join(s.split(":")[1] for s in header.values())) == set("iuldp")


def test_types_are_set_on_load(sharp):
    from sharp_amd import _abi

    L = sharp.lib()
    for name, sig in _abi.SIGNATURES.items():
        ret, args = sig.split(":")
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), name
        assert list(fn.argtypes) == [_abi.ARGUMENT[a] for a in args], name
        assert fn.restype is _abi.RETURN[ret], name
    assert all(t is C.c_void_p for t in L.sharp_tsne_gradient.argtypes[:3])           # every pointer is a void *, whatever it points to


# ---- every entry point's marshalling reaches the library ------------------------------------------------------------------------------
def _inputs():
    import scipy.sparse as sp

    rng = np.random.default_rng(0)
    X = rng.integers(0, 5, size=(30, 40)).astype(np.float64)
    idx = (np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40
    return {"X": X, "Xs": sp.csc_matrix(X), "E": rng.normal(size=(40, 6)), "lab": np.arange(40) % 3 + 1,
            "d": np.abs(rng.normal(size=780)) + 0.1, "idx": idx, "nd": rng.uniform(0.5, 2.0, size=(40, 3))}


_CALLS = {
    "ranM2": lambda s, v: s.ranM2(30, 5, 1),
    "get_opt_hclust": lambda s, v: s.get_opt_hclust(v["E"]),
    "getrowColor": lambda s, v: s.getrowColor(v["E"]),
    "wMetaC": lambda s, v: s.wMetaC(np.stack([v["lab"], v["lab"][::-1]], 1)),
    "sMetaC": lambda s, v: s.sMetaC(v["lab"], v["E"]),
    "SHARP-dense": lambda s, v: s.SHARP(v["X"], logflag=False),
    "SHARP-sparse": lambda s, v: s.SHARP(v["Xs"], logflag=False),
    "SHARP_small": lambda s, v: s.SHARP_small(v["X"]),
    "SHARP_unlimited-dense": lambda s, v: s.SHARP_unlimited([v["X"], v["X"]]),
    "SHARP_unlimited-devices": lambda s, v: s.SHARP_unlimited([v["X"], v["X"]], devices=[0]),
    "SHARP_unlimited-sparse": lambda s, v: s.SHARP_unlimited([v["Xs"], v["Xs"]]),
    "SHARP_unlimited2": lambda s, v: s.SHARP_unlimited2([v["X"], v["X"]], logflag=False),
    "get_marker_genes": lambda s, v: s.get_marker_genes(v["X"], v["lab"]),
    "Rtsne-exact": lambda s, v: s.Rtsne(v["E"], perplexity=5),
    "Rtsne-barnes_hut": lambda s, v: s.Rtsne(v["E"], perplexity=5, repulsion="barnes_hut"),
    "Rtsne-is_distance": lambda s, v: s.Rtsne(v["d"], perplexity=5, is_distance=True),
    "Rtsne_neighbors": lambda s, v: s.Rtsne_neighbors(v["idx"], v["nd"], perplexity=1),
    "knn-rows": lambda s, v: s.knn(v["E"], 3),
    "knn-is_distance": lambda s, v: s.knn(v["d"], 3, is_distance=True),
    "dist": lambda s, v: s.tree.dist(v["E"]),
    "hclust-x": lambda s, v: s.tree.hclust(x=v["E"]),
    "hclust-d": lambda s, v: s.tree.hclust(d=v["d"]),
    "silhouette-data": lambda s, v: s.validity.silhouette(v["lab"], data=v["E"]),
    "silhouette-d": lambda s, v: s.validity.silhouette(v["lab"], d=v["d"]),
    "calinski_harabasz": lambda s, v: s.validity.calinski_harabasz(v["E"], v["lab"]),
}


@pytest.mark.parametrize("name", list(_CALLS))
def test_marshalling_reaches_the_library(sharp, monkeypatch, name):
    """With the package told that device 0 is initialised, each call converts its arguments and enters the library, which has no context:
    its SharpError, never a ctypes.ArgumentError or a TypeError from the conversion."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sharp_amd.tree
    import sharp_amd.validity  # noqa: F401

    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    with pytest.raises(sharp.SharpError) as e:
        _CALLS[name](sharp, _inputs())
    assert "no device context" in str(e.value) or "no HIP device" in str(e.value)


def _device_calls():
    """sharp_amd.device's entry points take resident tensors; only the addresses travel, so CPU tensors carry the marshalling as far"""
    import torch

    from sharp_amd import device

    X = torch.zeros((300, 50), dtype=torch.float32)
    X64 = torch.zeros((300, 50), dtype=torch.float64)
    return {
        "synth_fill": lambda: device.synth_fill(X, 7, 0),
        "SHARP_dev": lambda: device.SHARP_dev(X, forview=True),
        "SHARP_dev-f64": lambda: device.SHARP_dev(X64, ensize_K=3, rN_seed=4),
        "unlimited_block_dev": lambda: device.unlimited_block_dev(X, 10, 0, 5, 1, viE=np.zeros((300, 10)), next_block=X),
        "unlimited_block_dev-f64": lambda: device.unlimited_block_dev(X64, 10, 0, 5, 1, viE=np.zeros((300, 10)), view_dim=10),
        "unlimited_blocks_dev": lambda: device.unlimited_blocks_dev([X, X64], 10, 0, 5, 1),
        "unlimited_dev": lambda: device.unlimited_dev([X, X], viewflag=True, rN_seed=3),
        "unlimited_merge": lambda: device.unlimited_merge(np.zeros((4, 3)), np.ones(4, np.int64), 100),
        "marker_genes_dev": lambda: device.marker_genes_dev(X, np.ones(300, np.int32), 2),
        "profile": lambda: device.profile(True),
    }


@pytest.mark.parametrize("name", ["synth_fill", "SHARP_dev", "SHARP_dev-f64", "unlimited_block_dev", "unlimited_block_dev-f64",
                                  "unlimited_blocks_dev", "unlimited_dev", "unlimited_merge", "marker_genes_dev", "profile"])
def test_device_marshalling_reaches_the_library(sharp, monkeypatch, name):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    with pytest.raises(sharp.SharpError, match="no device context|no HIP device"):
        _device_calls()[name]()


def test_last_decisions_without_a_device(sharp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rows = sharp.last_decisions()
    assert rows.shape == (0, 14)


# ---- refusals happen before the library -----------------------------------------------------------------------------------------------
def test_array_helper_checks_what_it_passes(sharp):
    from sharp_amd import _lib

    a = np.zeros((6, 4))
    assert _lib.ptr(None, np.float64) is None and _lib.f64(None) is None
    assert _lib.f64(a) == a.ctypes.data and _lib.f64(np.asfortranarray(a)) is not None
    assert _lib.i32(np.zeros(3, np.int32)) and _lib.i64(np.zeros(3, np.int64)) and _lib.i8(np.zeros(3, np.int8))
    with pytest.raises(TypeError, match="float64"):
        _lib.f64(np.zeros(4, np.int32))
    with pytest.raises(TypeError, match="float64"):
        _lib.f64(a[:, ::2])
    with pytest.raises(TypeError, match="int32"):
        _lib.i32(np.zeros(4, np.int64))
    with pytest.raises(TypeError, match="float64"):
        _lib.f64([0.0, 1.0])


def test_wrong_scalar_wrapper_is_refused(sharp):
    L = sharp.lib()
    with pytest.raises(C.ArgumentError):
        L.sharp_init(C.c_double(0))
    with pytest.raises(C.ArgumentError):
        L.sharp_init(C.c_longlong(0))
    with pytest.raises(C.ArgumentError):
        L.sharp_init(0.0)


def test_result_buffers_of_the_wrong_type_are_refused(sharp, monkeypatch):
    """A caller's result buffer goes to the library as double *: a float32 array of the right shape would be written past its end."""
    import torch

    from sharp_amd import device

    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    blocks = [torch.zeros((300, 50), dtype=torch.float32) for _ in range(2)]
    cols = int(np.ceil(np.log2(600) / 0.04))
    with pytest.raises(TypeError, match="float64"):
        device.unlimited_dev(blocks, viewflag=True, viE_out=np.zeros((600, cols), np.float32))
    pmax, cap = int(np.ceil(np.log2(300) / 0.04)), 42
    with pytest.raises(TypeError, match="float64"):
        device.SHARP_dev(blocks[0], forview=True, view_out=(np.zeros((300, pmax), np.float32), np.zeros(300 * cap, np.float32)))
    with pytest.raises(TypeError, match="float64"):
        device.SHARP_dev(blocks[0], forview=True, view_out=(np.zeros((300, 2 * pmax))[:, ::2], np.zeros(300 * cap)))
    with pytest.raises(TypeError, match="float64"):
        device.unlimited_block_dev(blocks[0], 10, 0, 5, 1, viE=np.zeros((300, 10), np.float32))
