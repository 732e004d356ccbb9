"""CPU: the host model of order_env (pgx_order_model.cpp, the step kernels' derivation of the
heavy-first env order from one key byte per env, lane for lane) against numpy's stable argsort,
for every wave of a segment."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "panda-gym_amd", "libpgx_order_model.so")
EPW = 4

SIZES = [1, 3, 63, 64, 65, 130, 256, 512, 1000, 1024]


@pytest.fixture(scope="module")
def model():
    assert os.path.exists(LIB), f"{LIB} missing: run __graft_entry__.build()"
    lib = C.CDLL(LIB)
    lib.pgx_order_model.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.pgx_order_model.restype = None
    return lib


def _patterns(S, rng):
    last = np.zeros(S, np.uint8)
    last[-1] = 12
    return {"all equal": np.full(S, 5, np.uint8),
            "a bin each": (np.arange(S) % 13).astype(np.uint8),   # every bin filled (as far as S reaches)
            "random": rng.integers(0, 13, S).astype(np.uint8),
            "heavy last": last}


def _order(lib, keys, n, segs, top=12):
    """The model's order of the whole batch: every wave's EPW slots (a ragged last wave's extra
    slots dropped, as the kernel's lanes with slot >= N leave)."""
    pad = np.full((n + 15) // 16 * 16, 0xAB, np.uint8)   # the padding holds anything: masked
    pad[:n] = keys
    nb = (n + EPW - 1) // EPW
    out = np.zeros(EPW, np.int32)
    order = np.full(nb * EPW, -1, np.int64)
    for b in range(nb):
        lib.pgx_order_model(pad.ctypes.data, n, segs, b, top, out.ctypes.data)
        # block b's slots: dispatch order under one segment, else XCD b % 8's range (xcd_block)
        blk = b if segs == 1 else (b % 8) * (nb // 8) + b // 8
        order[blk * EPW:(blk + 1) * EPW] = out
    return order[:n]


@pytest.mark.parametrize("S", SIZES)
def test_one_segment_matches_stable_argsort(model, S):
    rng = np.random.default_rng(S)
    for name, keys in _patterns(S, rng).items():
        want = np.argsort(-keys.astype(np.int64), kind="stable")
        got = _order(model, keys, S, 1)
        assert np.array_equal(got, want), (S, name)
    keys = rng.integers(0, 9, S).astype(np.uint8)   # the arm kernels' budget: bins 0..8
    assert np.array_equal(_order(model, keys, S, 1, top=8), np.argsort(-keys.astype(np.int64), kind="stable")), S


@pytest.mark.parametrize("S", [256, 512, 1024])
def test_eight_segments_each_match_stable_argsort(model, S):
    n = 8 * S
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 13, n).astype(np.uint8)
    keys[S - 1] = 12   # a heavy env at a segment's last index
    got = _order(model, keys, n, 8)
    for x in range(8):
        want = x * S + np.argsort(-keys[x * S:(x + 1) * S].astype(np.int64), kind="stable")
        assert np.array_equal(got[x * S:(x + 1) * S], want), (S, x)


def test_keys_outside_the_bins_stay_in_range(model):
    """Keys no epilogue writes (> 12) are ranked nowhere; the derived ids still lie in the segment."""
    n = 130
    keys = np.full(n, 200, np.uint8)
    keys[::3] = 4
    got = _order(model, keys, n, 1)
    assert got.min() >= 0 and got.max() < n
