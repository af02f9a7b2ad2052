"""The census of the evaluation kernels (tests/evalop_shapes.py) without a GPU:

* the table counts, the import-time assertions on the primes, and that the matrix reaches every reachable cell and
  every run-time coordinate under the restated dispatch rules on devices of 3, 64, 256 and 304 compute units;
* removing any one shape loses a cell or a coordinate of the table only if another shape does not reach it -- the
  shapes that alone reach something are named, so the census on the MI355X fails when one of them goes;
* the matrix shapes up to N = 2048 through tests/evalop_cases.py under host emulation of the kernel sources, against the
  C oracle, with `cus` = 3 (what the emulated device reports).  The emulation has no code objects, so which instance ran
  is not asserted here: tests/test_evalop_shapes_gpu.py reads it from the profiler's kernel symbols."""
import pytest

import evalop_cases as C
import evalop_shapes as S
from helpers import load_engine

EMU_CUS = 3
EMU_SHAPES = [s for s in S.matrix_shapes(EMU_CUS) if s.n <= 2048]


@pytest.fixture(scope="module")
def fhe():
    return load_engine("emu")


def test_table_counts():
    assert S.COUNTS == {"ntt_kernel": 82, "ntt_global_kernel": 4, "tensor_intt_kernel": 35, "ks_fused_kernel": 78,
                        "ks_fused_split_kernel": 8, "ks_ntt_kernel": 51, "ks_mac_kernel": 1}
    assert len(S.all_cells()) == 259
    assert S.UNREACHABLE == {}   # no family has an instance that is compiled and cannot be launched
    # every coordinate names a reachable cell
    assert {(f, a) for f, a, _c in S.required_coords()} <= S.all_cells()


@pytest.mark.parametrize("cus", [3, 64, 256, 304])
def test_matrix_reaches_every_cell(cus):
    symbols, coords = S.coverage(cus)
    assert sorted(S.all_cells() - symbols) == []
    assert sorted(symbols - S.all_cells()) == []
    assert sorted(S.required_coords() - coords) == []
    assert not symbols & set(S.UNREACHABLE)


@pytest.mark.parametrize("cus", [3, 256])
def test_every_shape_is_needed(cus):
    """A run that launches what the rules predict passes the census, and without any one shape it does not: every shape
    is the only one that reaches some cell or coordinate, and the census names what went missing."""
    shapes = S.matrix_shapes(cus)
    launched = {i: S.symbols_of(S.cells(s, cus)) for i, s in enumerate(shapes)}
    assert S.census(launched, shapes, cus) == ([], [], [])
    for i in range(len(shapes)):
        missing, foreign, coords = S.census({j: c for j, c in launched.items() if j != i}, shapes, cus)
        assert (missing or coords) and not foreign, ("the matrix does not need", shapes[i])
        own = {(f, a) for f, a, _c in S.cells(shapes[i], cus)}
        assert set(missing) | {(f, a) for f, a, _c in coords} <= own


def test_batches_follow_the_compute_units():
    """The issue's example: two 58-bit moduli at N = 8 extend to five rows; 3 * 5 * nb > 2 * 256 first holds at 35."""
    assert S.tensor_batch(5, 3, 256) == 35 and not S.tensor_fills(5, 34, 3, 256)
    assert S.tensor_batch(5, 14, 256) == 18 and S.tensor_batch(5, 16, 256) == 5 and S.tensor_batch(5, 15, 256) == 9
    assert S.tensor_batch(5, 3, 8) == 1 and S.tensor_batch(5, 3, 9) == 2
    for cus in (64, 256, 304):
        two = [s for s in S.matrix_shapes(cus) if s.what == "two workgroups per compute unit"]
        assert len(two) == 3 and all(s.batch * len(s.moduli) > cus >= (s.batch - 1) * len(s.moduli) for s in two)
        # rows above N = 16384: two or three moduli, small batches but for the derived tensor minimum
        for s in S.matrix_shapes(cus):
            if s.n > 16384:
                assert len(s.moduli) <= 3 and (s.batch <= 3 or s.what == "tensor launch of more than one round"), s


def test_lift_modes_of_the_chosen_primes():
    for kind in ("general", "narrow"):
        for n in (8, 4096, 65536):
            for lift in (0, 1, 2):
                q = S.moduli_for(kind, lift, n)
                assert S.lift_mode(q, q) == lift and S.ks_rns(q) == (lift == 1)
                assert (max(q) >> 60 != 0) == (kind == "general") and max(q) < (1 << 62)


@pytest.mark.parametrize("i", range(len(EMU_SHAPES)), ids=lambda i: "%d-%s" % (EMU_SHAPES[i].n, "+".join(EMU_SHAPES[i].ops)))
def test_matrix_shape(fhe, i):
    shape = EMU_SHAPES[i]
    assert S.cells(shape, EMU_CUS)     # (the prediction exists; the emulation cannot confirm it)
    C.check_shape(fhe, False, shape)
