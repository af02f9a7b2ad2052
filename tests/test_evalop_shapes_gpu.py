"""The census of the evaluation kernels on the MI355X (the HIP build): every shape of evalop_shapes.matrix_shapes(cus)
through evalop_cases.check_shape -- every compared word against the C oracle, F64-eligible shapes a second time on the
integer kernels -- with the profiler on; the kernel symbols of each run must name the cells evalop_shapes.cells()
predicts for it, and the union over the matrix must be the reachable table exactly, with nothing from UNREACHABLE.
`cus` is the device's compute-unit count, which the tensor rule and the 512-thread F64 key switch read."""
import pytest

import evalop_cases as C
import evalop_shapes as S
from helpers import HIP_LIB, load_engine

pytestmark = pytest.mark.gpu

# (the shapes of a 256-unit card number the parameters; the device's own count decides what runs)
N_MATRIX = len(S.matrix_shapes(256))


@pytest.fixture(scope="module")
def fhe():
    eng = load_engine("hip")
    from fhe_rs_amd import _lib
    assert _lib.loaded_path() == HIP_LIB, "GPU tests must run on the HIP build"
    assert eng.device_count() >= 1, "no HIP device visible"
    return eng


_launched = {}   # matrix index -> the (family, template arguments) its run launched


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def matrix():
    shapes = S.matrix_shapes(device_cus())
    assert len(shapes) == N_MATRIX, "the matrix of this device has another length than a 256-unit card's"
    return shapes


def run_matrix_shape(fhe, i):
    """Shape i with the profiler around it, as tests/test_devop_shapes_gpu.py's run_matrix_shape."""
    shape = matrix()[i]
    want = S.cells(shape, device_cus())
    assert fhe.get_f64()
    fhe.prof_reset()
    fhe.prof_enable(True)
    try:
        wants = C.case_shape(fhe, True, shape)
        symbols = [sym for _label, sym, _n, _ms in fhe.prof_entries()]
    finally:
        fhe.prof_enable(False)
        fhe.prof_reset()
    launched = {C.cell_of_symbol(s) for s in symbols} - {None}
    assert launched >= S.symbols_of(want), ("not launched", sorted(S.symbols_of(want) - launched), shape)
    assert not launched & set(S.UNREACHABLE), sorted(launched & set(S.UNREACHABLE))
    _launched[i] = launched
    if S.f64_eligible(shape):   # the same calls on the integer kernels: the same words
        fhe.set_f64(False)
        try:
            C.case_shape(fhe, True, shape, wants)
        finally:
            fhe.set_f64(True)


@pytest.mark.parametrize("i", range(N_MATRIX))
def test_matrix_shape(fhe, i):
    run_matrix_shape(fhe, i)


def test_matrix_launches_every_instance(fhe):
    """The union over the matrix equals the reachable table, the run-time coordinates are covered and no UNREACHABLE
    symbol ran (shapes that did not run in this process yet -- a selected or distributed run -- run here)."""
    for i in range(N_MATRIX):
        if i not in _launched:
            run_matrix_shape(fhe, i)
    missing, foreign, coords = S.census(_launched, matrix(), device_cus())
    assert not missing, ("never launched", missing)
    assert not foreign, ("launched but in no table", foreign)
    assert not coords, ("coordinates not covered", coords)
    assert len(set().union(*_launched.values())) == 259
