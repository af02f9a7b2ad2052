"""The multiparty share kernels on the MI355X (the HIP build) beyond the stock parameter sets:

* every shape of devop_shapes.matrix_shapes() through mbfv_shape_cases.case_shape -- every word of every share against the
  restatement (tests/mbfv_ref.py), at level 0 and the deepest level, the relin rounds on --, F64-eligible shapes a second
  time on the integer kernels; the profiler's kernel symbols over that run must name every one of the 33 x 3
  (mbfv_share_kernel, LOGM, kind, form) instances;
* batches that span launch groups: the first item, the last item and both neighbours of every boundary against the
  restatement, and the whole batch against the same call made in two parts (mbfv_shape_cases.split_invariant), for every
  share, the aggregator and fhe_mbfv_decrypt_dev.  Every split is derived from the group rule and asserted to exist
  before anything runs;
* the first 16 shapes of the `mbfv` family of tests/random_sweep_gpu.py."""
import pytest

import devop_cases as D
import devop_shapes as S
import encode_cases as E
import mbfv_shape_cases as M
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

N_MATRIX = 2 * 12 + 3 * 3


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


_matrix = []
_launched = {}   # matrix index -> the cells its run launched


def matrix():
    if not _matrix:
        _matrix.extend(S.matrix_shapes())
        assert len(_matrix) == N_MATRIX and all(len(s[1]) >= 2 for s in _matrix)   # (two moduli: the relin rounds run)
    return _matrix


def run_matrix_shape(fhe, i):
    """Shape i with the profiler around it, as tests/test_devop_shapes_gpu.py's run_matrix_shape."""
    shp = matrix()[i]
    assert fhe.get_f64()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        M.case_shape(fhe, True, shp)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    cells = {D.mbfv_cell_of_symbol(s) for s in symbols} - {None}
    assert cells >= S.mbfv_cells(shp), ("not launched", sorted(S.mbfv_cells(shp) - cells), shp)
    _launched[i] = cells
    if D.mbfv_f64_eligible(shp):   # the same launches on the integer kernels: the same bits
        fhe.set_f64(False)
        try:
            M.case_shape(fhe, True, shp)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    run_matrix_shape(fhe, i)


def test_matrix_launches_every_instance(fhe):
    """Every (mbfv_share_kernel, LOGM, kind, form) cell appears among the kernel symbols of the matrix run (shapes that
    did not run in this process yet -- a selected or distributed run -- run here)."""
    for i in range(N_MATRIX):
        if i not in _launched:
            run_matrix_shape(fhe, i)
    seen = set().union(*_launched.values())
    missing = sorted(S.mbfv_all_cells() - seen)
    assert not missing, missing
    assert len(seen & S.mbfv_all_cells()) == 99


# ---- launch-group boundaries -------------------------------------------------------------------------------------------
# The smallest shapes at which the boundaries exist: N = 8 over [62, 60] (general instances) for whole rows, N = 32768
# over two moduli for rows larger than one LDS tile.
NO_BUDGET = 1 << 62
WHOLE_BATCH = 65537
LARGE_N, LARGE_SIZES = 32768, [55, 60]


def share_group(nmoduli, n, edraws, batch):
    """Items per launch group of mbfv_shares (engine.hpp), through the restated encrypt_group: whole rows (N <= 16384)
    count 1 row per item against no byte budget, so only the cap of 65535 items a launch splits a batch; for
    N >= 32768 the transformed draws, `edraws` rows per item, stay within 256 MiB.  Either way the batch is cut into
    groups of equal size."""
    if n <= 16384:
        return D.launch_group(nmoduli, n, 1, batch, NO_BUDGET)
    return D.launch_group(nmoduli, n, edraws, batch, 256 << 20)


def small(fhe):
    return E.params(fhe, 8, 1153, moduli_sizes=[62, 60])


def large(fhe):
    return E.params(fhe, LARGE_N, E.stock_t(LARGE_N), moduli_sizes=LARGE_SIZES)


@pytest.mark.parametrize("kind", ["pk", "dec", "dec_shared", "sks", "rlk"])
def test_whole_row_groups(fhe, kind):
    """Batch 65537 at N = 8: more than the 65535 items one launch takes, so mbfv_shares cuts it into two groups of equal
    size.  A secret per item; "dec_shared": one secret and 65537 ciphertexts."""
    opar, par = small(fhe)
    L, batch = len(opar.moduli), WHOLE_BATCH
    g = share_group(L, 8, 2 * L if kind == "rlk" else 1, batch)
    assert 1 < g < batch and -(-batch // g) == 2
    items = D.boundary_items(batch, g)
    assert items == [0, g - 1, g, batch - 1]
    cut = batch // 3
    assert cut % g and cut < 65535 and batch - cut < 65535   # (each part is one group)
    M.case_share_groups(fhe, True, opar, par, kind, batch, items, cut)


def test_whole_row_groups_public_key_switch(fhe):
    """The public-key-switch share is encrypt_pk with an addend: whole rows go in launches of 65535 items and a tail."""
    opar, par = small(fhe)
    batch = WHOLE_BATCH
    g = D.chunk_group(batch)
    assert 1 < g < batch and -(-batch // g) == 2
    items = D.boundary_items(batch, g)
    assert items == [0, g - 1, g, batch - 1] and batch - g == 2
    cut = batch // 3
    assert cut % g and batch - cut < g
    M.case_share_groups(fhe, True, opar, par, "pks", batch, items, cut)


@pytest.mark.parametrize("kind", ["dec", "sks", "pks", "rlk"])
def test_large_row_groups(fhe, kind):
    """N = 32768 over two moduli, P parties x one ciphertext: one item more than the 256 MiB of transformed draws hold
    (1 draw per item for the decryption and secret-key-switch shares, 3 for the public-key-switch share, 2L = 4 for
    the relin rounds), so every share is made in two groups."""
    opar, par = large(fhe)
    L = len(opar.moduli)
    rows = {"dec": 1, "sks": 1, "pks": 3, "rlk": 2 * L}[kind]
    most = (256 << 20) // (rows * L * LARGE_N * 8)
    batch = most + 1
    g = share_group(L, LARGE_N, rows, batch)
    assert 1 < g < batch and -(-batch // g) == 2
    items = D.boundary_items(batch, g)
    assert items == [0, g - 1, g, batch - 1]
    cut = batch // 3
    assert cut % g and cut <= most and batch - cut <= most   # (each part is one group)
    M.case_share_groups(fhe, True, opar, par, kind, batch, items, cut)


def test_aggregator_groups(fhe):
    """65537 polynomials of N = 8 over [62, 62], 4 shares (one past the lazy window of 3)."""
    opar, par = E.params(fhe, 8, 1153, moduli_sizes=[62, 62])
    assert all(int(m).bit_length() == 62 for m in par.moduli)
    npolys = WHOLE_BATCH
    g = D.chunk_group(npolys)
    assert 1 < g < npolys and -(-npolys // g) == 2
    M.case_sum_groups(fhe, True, par, 8, npolys, nshares=4)


def test_decrypt_groups(fhe):
    """fhe_mbfv_decrypt_dev at batch 65537, 3 parties: the aggregator's launches of 65535 polynomials read the base at a
    stride of 2 L N words."""
    opar, par = small(fhe)
    batch = WHOLE_BATCH
    g = D.chunk_group(batch)
    assert 1 < g < batch
    items = D.boundary_items(batch, g)
    assert items == [0, g - 1, g, batch - 1]
    M.case_decrypt_groups(fhe, True, opar, par, batch, items, parties=3)


# ---- the fixed head of the sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(16))
def test_random_shape(fhe, idx):
    M.case_random_shape(fhe, True, idx)
