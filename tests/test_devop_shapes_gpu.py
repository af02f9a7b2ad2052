"""Device encode, encrypt and key generation on the MI355X (the HIP build) beyond the stock parameter sets:

* every shape of devop_shapes.matrix_shapes() through the parity cases (tests/devop_cases.py), every item against the
  restatements bit for bit, F64-eligible shapes a second time on the integer kernels; the profiler's kernel symbols
  over that run must name every one of the 7 x 33 (kernel, LOGM, kind) instances;
* round trips through the engine's and the oracle's decryption on a general shape, a class-3 shape and a 61-bit t;
* batches that span launch groups (the first item, the last item and both neighbours of every boundary, computed
  from the group rule), variances 1 ... 32 on whole rows, and draws that end inside a word;
* the first 32 shapes of the `devops` family of tests/random_sweep_gpu.py."""
import pytest

import devop_cases as D
import devop_shapes as S
import encode_cases as E
import encrypt_cases as X
import keygen_cases as G
import ref_params
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
        assert len(_matrix) == N_MATRIX
    return _matrix


def run_matrix_shape(fhe, i):
    """Shape i with the profiler around it: the entries are read (and the table cleared) per shape, which also returns
    the launches' events to the pool; the union over the shapes is the matrix run's."""
    shp = matrix()[i]
    first_of_logm = i == min(j for j, s in enumerate(matrix()) if s[0] == shp[0])
    assert fhe.get_f64()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        D.check_shape(fhe, True, shp, host_handle=first_of_logm)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    cells = {D.cell_of_symbol(s) for s in symbols} - {None}
    assert cells >= S.cells(shp), ("not launched", sorted(S.cells(shp) - cells), shp)
    _launched[i] = cells
    if D.f64_eligible(shp):   # the same launches on the integer kernels: the same bits
        fhe.set_f64(False)
        try:
            D.check_shape(fhe, True, shp)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    run_matrix_shape(fhe, i)


def test_matrix_launches_every_instance(fhe):
    """Every (kernel, LOGM, kind) cell appears among the kernel symbols of the matrix run (shapes that did not run in
    this process yet -- a selected or distributed run -- run here)."""
    for i in range(N_MATRIX):
        if i not in _launched:
            run_matrix_shape(fhe, i)
    seen = set().union(*_launched.values())
    missing = sorted(S.all_cells() - seen)
    assert not missing, missing
    assert len(seen & S.all_cells()) == 231


@pytest.mark.parametrize("i", range(3), ids=["general", "class3", "t61"])
def test_roundtrip(fhe, i):
    opar, par = D.params(fhe, S.roundtrip_shapes()[i])
    X.case_roundtrip(fhe, True, opar, par, level=0)


# ---- launch-group boundaries -------------------------------------------------------------------------------------------
def test_encrypt_groups_stock_16384(fhe):
    """Batch 1024 at stock n = 16384, level 0: the secret-key form splits its 1 GiB of seeded `a` rows into groups."""
    n, batch = 16384, 1024
    opar, par = E.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])
    g = D.launch_group(len(opar.moduli), n, 1, batch, 1 << 30)
    assert 1 < g < batch
    items = D.boundary_items(batch, g)
    assert items == [0, g - 1, g, batch - 1]
    X.case_encrypt_parity(fhe, True, opar, par, levels=[0], batch=batch, check_items=lambda b: items, seed=13,
                          modes=("each", "shared"))


def test_encrypt_groups_rows_larger_than_lds(fhe):
    """N = 32768: one item more than twice the 256 MiB group of the public-key form (three transformed sample rows
    per item); the secret-key form (two rows per item) splits the same batch elsewhere."""
    n, sizes = 32768, [50, 55, 60]
    opar, par = E.params(fhe, n, E.stock_t(n), moduli_sizes=sizes)
    L = len(sizes)
    most_pk = (256 << 20) // (3 * L * n * 8)
    batch = 2 * most_pk + 1
    g_pk, g_sk = D.launch_group(L, n, 3, batch, 256 << 20), D.launch_group(L, n, 2, batch, 256 << 20)
    assert 1 < g_pk < batch and 1 < g_sk < batch and -(-batch // g_pk) == 3
    items = sorted(set(D.boundary_items(batch, g_pk)) | set(D.boundary_items(batch, g_sk)))
    X.case_encrypt_parity(fhe, True, opar, par, levels=[0], batch=batch, check_items=lambda b: items, seed=14,
                          modes=("each",))


def test_keygen_groups_stock_4096(fhe):
    n, nkeys = 4096, 40
    opar, par = G.params(fhe, n, ref_params.plaintext_modulus(n), moduli=ref_params.DEFAULT_128[n])
    L = len(opar.moduli)
    g = D.launch_group(L, n, L, nkeys, 1 << 30, D.KG_KEYS)
    assert 1 < g < nkeys
    exps = [pow(3, i, 2 * n) for i in range(nkeys)]
    G.case_galois(fhe, True, opar, par, exps, 0, 0, check=set(D.boundary_items(nkeys, g)))


def test_keygen_groups_rows_larger_than_lds(fhe):
    n, sizes, nkeys = 32768, [50, 55], 33
    opar, par = G.params(fhe, n, E.stock_t(n), moduli_sizes=sizes)
    L = len(sizes)
    g = D.launch_group(L, n, 2 * L, nkeys, 256 << 20, D.KG_KEYS)
    assert 1 < g < nkeys
    exps = [pow(3, i, 2 * n) for i in range(nkeys)]
    G.case_galois(fhe, True, opar, par, exps, 0, 0, check=set(D.boundary_items(nkeys, g)))


# ---- variances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 16, 17, 32])
def test_variances_whole_rows(fhe, v):
    """N = 4096 over [62, 45, 36] (general instances): the packed draws (v <= 16) and the two-word draws (v > 16)."""
    opar, par = D.params(fhe, S.shape(4096, [62, 45, 36], 55, v, 2))
    assert S.row_kind(opar.moduli, 12) == "general"
    X.case_encrypt_parity(fhe, True, opar, par, batch=2, seed=60 + v)
    G.case_relin(fhe, True, opar, par, 0, 0, seed=70 + v)


@pytest.mark.parametrize("v", [3, 17])
def test_draws_start_at_word_boundaries(fhe, v):
    """N = 8 with odd v: a draw of 8 samples ends inside a word and the next draw starts at the next one
    (tests/test_encrypt_emu.py runs the same on the emulation)."""
    opar, par = G.params(fhe, 8, 1153, moduli_sizes=[62, 60], variance=v)
    assert (8 * 4 * v) % 64 != 0 or v > 16
    X.case_sampler_parity(fhe, True, opar, par, (v,), batch=2)
    X.case_encrypt_parity(fhe, True, opar, par, batch=3)


# ---- the fixed head of the sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(32))
def test_random_shape(fhe, idx):
    D.check_random_shape(fhe, True, idx)
