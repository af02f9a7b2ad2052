"""Key-switching keys from and to their wire bytes on the MI355X (the HIP build), against tests/keyload_ref.py:

* the 33 matrix shapes of tests/devop_shapes.py, seeded and unseeded; the profiler's kernel symbols over that run must
  name all 33 (LOGM, kind) instances of ksk_load_kernel; F64-eligible shapes a second time on the integer kernels;
* rows at odd byte offsets (N = 8, three bit lengths, a pointer one byte past its allocation), both sides of the
  word-path threshold (N = 64, 128; aligned and misaligned), a decomposition key, rows above one LDS tile (N = 32768),
  one key more than a launch group, the key types, the range check and every status."""
import re

import pytest

import devop_cases as D
import devop_shapes as S
import encode_cases as E
import keygen_cases as G
import keyload_cases as K
import keyload_ref as KR
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

N_MATRIX = 2 * 12 + 3 * 3
KERNEL = "ksk_load_kernel"


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


def params(fhe, n, sizes, t=None):
    return G.params(fhe, n, t or E.stock_t(n), moduli_sizes=sizes)


# ---- every instance ----------------------------------------------------------------------------------------------------
_SYMBOL = re.compile(r"(ksk_load_kernel)<(\d+), (true|false), (\d+)>")
_matrix = []
_launched = {}   # matrix index -> the (LOGM, kind) cells its run launched


def cell_of_symbol(symbol):
    m = _SYMBOL.search(symbol)
    if not m:
        return None
    hr = int(m.group(4))
    return int(m.group(2)), "f64_%d" % hr if hr else "narrow" if m.group(3) == "true" else "general"


def all_cells():
    return {(lm, k) for kern, lm, k in S.all_cells() if kern == "ksk_gen_kernel"}


def matrix():
    if not _matrix:
        _matrix.extend(S.matrix_shapes())
        assert len(_matrix) == N_MATRIX
    return _matrix


def run_matrix_shape(fhe, i):
    shp = matrix()[i]
    n = shp[0]
    lm = n.bit_length() - 1
    opar, par = D.params(fhe, shp)
    want = (lm, S.row_kind(opar.moduli, lm))   # the key context is level 0's
    first_of_logm = i == min(j for j, s in enumerate(matrix()) if s[0] == n)
    assert fhe.get_f64()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        K.case_load(fhe, True, opar, par, 0, 0, switch=first_of_logm or n <= 2048)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    cells = {cell_of_symbol(s) for s in symbols} - {None}
    assert want in cells, ("not launched", want, sorted(cells), shp)
    _launched[i] = cells
    if want[1].startswith("f64"):   # the same loads on the integer kernels: the same bits
        fhe.set_f64(False)
        try:
            K.case_load(fhe, True, opar, par, 0, 0, switch=False)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    run_matrix_shape(fhe, i)


def test_matrix_launches_every_instance(fhe):
    """Every (LOGM, kind) instance of ksk_load_kernel appears among the kernel symbols of the matrix run (shapes that
    did not run in this process yet -- a selected or distributed run -- run here)."""
    for i in range(N_MATRIX):
        if i not in _launched:
            run_matrix_shape(fhe, i)
    seen = set().union(*_launched.values())
    missing = sorted(all_cells() - seen)
    assert not missing, missing
    assert len(seen & all_cells()) == 33


# ---- the loader's paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "offset1"])
def test_rows_at_odd_byte_offsets(fhe, misalign):
    """N = 8 over moduli of three bit lengths: a row is nbits bytes, so rows start at odd offsets (the byte path)."""
    opar, par = params(fhe, 8, [61, 35, 27], 1153)
    assert [KR.wire_bits(q) for q in opar.ctx[0].moduli] == [61, 35, 27]
    K.case_load(fhe, True, opar, par, 0, 0, misalign=misalign)


@pytest.mark.parametrize("n,misalign", [(64, False), (64, True), (128, False), (128, True)])
def test_word_path_threshold(fhe, n, misalign):
    """N = 64 always reads bytes; N = 128 reads words from an aligned pointer and bytes from a misaligned one."""
    opar, par = params(fhe, n, [62, 53, 36])
    K.case_load(fhe, True, opar, par, 0, 0, misalign=misalign)


@pytest.mark.parametrize("sizes", [[62, 45], [50, 44]], ids=["general", "f64"])
def test_misaligned_pointer_whole_rows_8192(fhe, sizes):
    """A caller's pointer at any address at a size whose aligned loads go through the transform's loader."""
    opar, par = params(fhe, 8192, sizes)
    K.case_load(fhe, True, opar, par, 0, 0, misalign=True, switch=False)


def test_decomposition_key_8_points(fhe):
    opar, par = params(fhe, 8, [45], 1153)
    assert KR.key(opar, 0, 0, 1)["lb"] != 0
    K.case_load(fhe, True, opar, par, 0, 0, misalign=True)


def test_key_level_below_ciphertext_level(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_load(fhe, True, opar, par, 1, 0)
    K.case_single(fhe, True, opar, par)


def test_rows_larger_than_lds(fhe):
    """N = 32768 over two moduli: wire_deserialize into the handle, launch_ntt, then the element-wise twins."""
    opar, par = params(fhe, 32768, [50, 55])
    K.case_load(fhe, "abi", opar, par, 0, 0)


def test_one_more_key_than_a_launch_group(fhe):
    """33 keys at N = 8: the group rule splits them 17 + 16; both neighbours of the boundary and the ends."""
    opar, par = params(fhe, 8, [62, 60], 1153)
    nkeys = D.KG_KEYS + 1
    g = D.launch_group(2, 8, 2, nkeys, 1 << 30, D.KG_KEYS)
    assert g == 17 and D.boundary_items(nkeys, g) == [0, 16, 17, 32]
    K.case_load(fhe, True, opar, par, 0, 0, key_seeds=tuple(range(100, 100 + nkeys)), check={0, 16, 17, 32})


# ---- the public interface ----------------------------------------------------------------------------------------------
def test_generated_key_round_trip(fhe):
    opar, par = params(fhe, 4096, [50, 50, 40])
    K.case_generated_to_wire(fhe, True, opar, par)


@pytest.mark.parametrize("n,sizes", [(16, [62, 60, 55]), (4096, [50, 50, 40])], ids=["16", "4096_f64"])
def test_key_types(fhe, n, sizes):
    opar, par = params(fhe, n, sizes, 1153 if n == 16 else None)
    K.case_types(fhe, True, opar, par)


@pytest.mark.parametrize("n,sizes", [(8, [61, 35, 27]), (128, [62, 53]), (8, [45]), (8192, [50, 44])],
                         ids=["bytes", "words", "decomposition", "loader_f64"])
def test_range_check(fhe, n, sizes):
    opar, par = params(fhe, n, sizes, 1153 if n == 8 else None)
    K.case_range(fhe, True, opar, par)


def test_range_check_rows_larger_than_lds(fhe):
    opar, par = params(fhe, 32768, [50, 55])
    K.case_range(fhe, "abi", opar, par, nkeys=1)


def test_statuses(fhe):
    opar, par = params(fhe, 16, [62, 60, 55], 1153)
    K.case_statuses(fhe, True, opar, par)
