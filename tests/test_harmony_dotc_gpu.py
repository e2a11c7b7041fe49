"""sharp_C_harmony called the way R's .C() calls a native routine (every argument a pointer into a caller-owned vector, the status last):
the plain entry's bits.  This is the call r/sharp_hip.R makes."""
import ctypes as C

import numpy as np
import pytest

import _harmony_ref as hr

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


def dotc(lib, name, *args):
    getattr(lib, name)(*[P(a) for a in args])


def last_error(lib):
    buf = C.create_string_buffer(b" " * 2047)
    ptr = (C.c_char_p * 1)(C.addressof(buf))
    lib.sharp_C_last_error(ptr, P(I(2048)))
    return buf.value.decode()


def test_dotc_harmony(sa):
    Z, b, _ = hr.planted(400)
    n, d, K, B, iters = 400, 10, 12, 3, 4
    want = sa.harmony_integrate(Z, b, n_clusters=K, max_iter=iters, max_iter_cluster=6, n_blocks=7, seed=3, ret_R=True)
    b32 = b.astype(np.int32)
    for want_R in (1, 0):
        Zc, Y, obj, rounds, ni, cv, st = np.zeros(n * d), np.zeros(K * d), np.zeros(iters), np.zeros(iters, np.int32), I(0), I(0), I(-1)
        R = np.zeros(n * K) if want_R else D(-7.0)
        dotc(sa.lib(), "sharp_C_harmony", Z, D(n), I(d), b32, I(B), I(K), D(0.1), D(2.0), D(1.0), I(iters), I(6), I(7), D(1e-5), D(1e-4), I(10), D(3),
             Zc, Y, obj, rounds, ni, cv, I(want_R), R, st)
        assert st[0] == 0, last_error(sa.lib())
        assert Zc.tobytes() == want["Z_corr"].tobytes() and Y.tobytes() == want["Y"].tobytes()
        assert ni[0] == want["n_iter"] and bool(cv[0]) == want["converged"]
        assert obj[:ni[0]].tobytes() == want["objective"].tobytes() and np.array_equal(rounds[:ni[0]], want["rounds"])
        if want_R:
            assert R.tobytes() == want["R"].tobytes()
        else:
            assert R[0] == -7.0                                                  # left alone
    dotc(sa.lib(), "sharp_C_harmony", Z, D(n), I(d), np.zeros(n, np.int32), I(1), I(K), D(0.1), D(2.0), D(1.0), I(iters), I(6), I(7), D(1e-5), D(1e-4),
         I(10), D(3), Zc, Y, obj, rounds, ni, cv, I(0), D(0.0), st)
    assert st[0] != 0 and "harmony_integrate: one batch: nothing to integrate" in last_error(sa.lib())
    dotc(sa.lib(), "sharp_C_harmony", Z, D(n), I(d), b32, I(B), I(401), D(0.1), D(2.0), D(1.0), I(iters), I(6), I(7), D(1e-5), D(1e-4), I(10), D(3), Zc,
         Y, obj, rounds, ni, cv, I(0), D(0.0), st)
    assert st[0] != 0 and "harmony_integrate: n_clusters exceeds the number of cells" in last_error(sa.lib())
