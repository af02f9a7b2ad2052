"""Plaintexts from packed bits on the MI355X (the HIP build), against tests/transcode_ref.py:

* the case functions of tests/test_transcode_emu.py on the device;
* the 33 matrix shapes of tests/devop_shapes.py through encode_bytes and encode_words; the profiler's kernel symbols over
  that run must name all 33 (LOGM, kind) instances of encode_stream_kernel; F64-eligible shapes a second time on the
  integer kernels;
* one SealPIR round at N = 4096 with the examples' parameters."""
import random
import re

import numpy as np
import pytest

import devop_cases as D
import devop_shapes as S
import transcode_cases as TC
from fhe_oracle import coracle
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

N_MATRIX = 2 * 12 + 3 * 3
SMALL = [62, 60, 55]
THREE = [62, 52, 40]


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def shape(fhe, n, sizes, t_bits):
    return TC.params(fhe, n, TC.plaintext_modulus(t_bits, n, sizes), sizes)


# ---- every instance ----------------------------------------------------------------------------------------------------
_SYMBOL = re.compile(r"(encode_stream_kernel)<(\d+), (true|false), (\d+)>")
_matrix = []
_launched = {}   # matrix index -> the (LOGM, kind) cells its run launched


def cell_of_symbol(symbol):
    m = _SYMBOL.search(symbol)
    if not m:
        return None
    hr = int(m.group(4))
    return int(m.group(2)), "f64_%d" % hr if hr else "narrow" if m.group(3) == "true" else "general"


def all_cells():
    return {(lm, k) for kern, lm, k in S.all_cells() if kern == "encode_lift_kernel"}


def matrix():
    if not _matrix:
        _matrix.extend(S.matrix_shapes())
        assert len(_matrix) == N_MATRIX
    return _matrix


def matrix_case(fhe, opar, par, batch, seed):
    """encode_bytes (an odd item size, a short last item, one item past the end) and encode_words (the examples' widths,
    two segments of N words: the join inside a plaintext) at level 0 unscaled and at the deepest level scaled."""
    rng = random.Random(seed)
    n, t = opar.degree(), opar.plaintext
    nbits = TC.ilog2(t)
    enc = par.encoder()
    ib = min(n * nbits // 8, 1001)
    for level, scaled in ((0, False), (opar.max_level(), True)):
        cctx = coracle.CCtx(opar.ctx[level])
        data = TC.rand_bytes(rng, batch * ib + ib // 3)
        TC.check_bytes(fhe, True, opar, enc, cctx, data, ib, nbits, batch + 2, level, scaled, what=(n, t, level))
        w = np.array([[[rng.getrandbits(64) for _ in range(n)] for _ in range(2)] for _ in range(batch)], dtype=np.uint64)
        TC.check_words(fhe, True, opar, enc, cctx, w, 36, min(nbits, 20), level, scaled, what=(n, t, level))


def run_matrix_shape(fhe, i):
    shp = matrix()[i]
    n, batch = shp[0], shp[4]
    lm = n.bit_length() - 1
    opar, par = D.params(fhe, shp)
    want = (lm, S.row_kind(opar.moduli, lm))
    assert fhe.get_f64()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        matrix_case(fhe, opar, par, batch, i)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    cells = {cell_of_symbol(s) for s in symbols} - {None}
    assert want in cells, ("not launched", want, sorted(cells), shp)
    _launched[i] = cells
    if want[1].startswith("f64"):   # the same encodings on the integer kernels: the same bits
        fhe.set_f64(False)
        try:
            matrix_case(fhe, opar, par, batch, i)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    run_matrix_shape(fhe, i)


def test_matrix_launches_every_instance(fhe):
    """Every (LOGM, kind) instance of encode_stream_kernel appears among the kernel symbols of the matrix run (shapes
    that did not run in this process yet -- a selected or distributed run -- run here)."""
    for i in range(N_MATRIX):
        if i not in _launched:
            run_matrix_shape(fhe, i)
    seen = set().union(*_launched.values())
    missing = sorted(all_cells() - seen)
    assert not missing, missing
    assert len(seen & all_cells()) == 33


# ---- the case functions of the emulated suite --------------------------------------------------------------------------
@pytest.mark.parametrize("in_bits", TC.WIDTHS)
def test_transcode_every_pair(fhe, in_bits):
    TC.case_transcode(fhe, True, in_widths=(in_bits,), seed=in_bits)


def test_transcode_shapes_and_counts(fhe):
    TC.case_transcode_misc(fhe, True)


@pytest.mark.parametrize("t_bits", (2, 14, 21, 34, 61))
@pytest.mark.parametrize("n,sizes", [(8, SMALL), (16, SMALL), (256, THREE)], ids=["8", "16", "256"])
def test_encode_bytes(fhe, n, sizes, t_bits):
    opar, par = shape(fhe, n, sizes, t_bits)
    TC.case_encode_bytes(fhe, True, opar, par, seed=n + t_bits)


@pytest.mark.parametrize("n,sizes,t_bits", [(4096, [36, 36, 37], 21), (8192, [62, 45], 21)], ids=["4096_f64", "8192_general"])
def test_encode_bytes_offsets_whole_rows(fhe, n, sizes, t_bits):
    """A source at byte offsets 1 and 7 at sizes where the interior of an item takes the aligned 8-byte loads."""
    opar, par = shape(fhe, n, sizes, t_bits)
    enc = par.encoder()
    rng = random.Random(n)
    ib = n * 20 // 8 - 3
    data = TC.rand_bytes(rng, ib + ib // 2)
    for off in (1, 7):
        TC.check_bytes(fhe, True, opar, enc, None, data, ib, 20, 2, 0, False, off=off, what=(n, off))


def test_encode_bytes_defaults(fhe):
    opar, par = shape(fhe, 16, SMALL, 21)
    TC.case_encode_bytes_defaults(fhe, True, opar, par)


@pytest.mark.parametrize("t_bits", [21, 34])
def test_encode_words(fhe, t_bits):
    opar, par = shape(fhe, 16, SMALL, t_bits)
    seen = TC.case_encode_words(fhe, True, opar, par, seg_lens=(5, 37))
    assert seen[(36, 20, 2, 16)] == 4


def test_statuses(fhe):
    import bigt_cases as B
    opar, par = shape(fhe, 16, SMALL, 21)
    _obig, par_big = B.params(fhe, "C", 16)
    TC.case_statuses(fhe, True, opar, par, par_big)


def test_rows_larger_than_lds(fhe):
    n = 32768
    opar, par = TC.params(fhe, n, 2056193, [50, 55])
    enc = par.encoder()
    cctx = coracle.CCtx(opar.ctx[0])
    rng = random.Random(7)
    ib = 1001
    TC.check_bytes(fhe, True, opar, enc, cctx, TC.rand_bytes(rng, ib + 333), ib, 20, 2, 0, True, what="32768 bytes")
    w = np.array([[[rng.getrandbits(64) for _ in range(n)] for _ in range(2)] for _ in range(2)], dtype=np.uint64)
    assert TC.check_words(fhe, True, opar, enc, cctx, w, 36, 20, 0, False, what="32768 words") == 4


# ---- SealPIR -----------------------------------------------------------------------------------------------------------
def test_sealpir_round_64(fhe):
    assert TC.case_sealpir_round(fhe, True, 64) == 4


def test_sealpir_round_4096(fhe):
    """The examples' parameters: N = 4096, t = 2056193, moduli of 36, 36 and 37 bits, 288-byte elements."""
    assert TC.case_sealpir_round(fhe, True, 4096, element_size=288) == 4
