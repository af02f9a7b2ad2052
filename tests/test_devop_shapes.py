"""The shape table of tests/devop_shapes.py: the oracle accepts every shape, and the matrix list reaches every
(kernel, LOGM, kind) instance of the seven whole-row encode / encrypt / key-generation kernels -- 7 x 33 = 231 cells,
derived here from the shapes' own moduli by the dispatch rules, restated below; the same for the 33 x 3 = 99 instances of
the multiparty share kernel.  No engine, no GPU."""
import devop_shapes as S
from fhe_oracle import bfv as obfv

ROW_KERNELS = ["encode_lift_kernel", "small_ntt_kernel", "encrypt_sk_kernel", "encrypt_pk_kernel"]
T_KERNELS = ["encode_simd_t_kernel", "decode_simd_kernel"]


def kind(moduli, logm):
    """Ctx::f64_class / f64_rows, Ctx::below_2p60 and with_row_kind: whole rows of 2^12 ... 2^14 points whose widest
    modulus is below 2^50 take the F64 class 5 (below 2^48), 4 (below 2^49) or 3; every other launch is narrow when all
    moduli are below 2^60 and general otherwise."""
    mx = max(moduli)
    if 12 <= logm <= 14 and not mx >> 50:
        return "f64_3" if mx >> 49 else "f64_4" if mx >> 48 else "f64_5"
    return "narrow" if all(not m >> 60 for m in moduli) else "general"


def required_cells():
    cells = set()
    for kernel in ROW_KERNELS + T_KERNELS + ["ksk_gen_kernel"]:
        for logm in range(3, 15):
            cells |= {(kernel, logm, "general"), (kernel, logm, "narrow")}
        for logm in (12, 13, 14):
            cells |= {(kernel, logm, "f64_%d" % hr) for hr in (3, 4, 5)}
    return cells


def launched_cells(opar):
    """What tests/devop_cases.py launches for one parameter set: the lift, the sampler and both encryptions over the
    moduli of level 0 and of the deepest level, key generation over the level-0 moduli, both transforms mod t."""
    logm = opar.degree().bit_length() - 1
    cells = {(k, logm, kind([opar.plaintext], logm)) for k in T_KERNELS}
    for level in (0, opar.max_level()):
        cells |= {(k, logm, kind(opar.ctx[level].moduli, logm)) for k in ROW_KERNELS}
    cells.add(("ksk_gen_kernel", logm, kind(opar.moduli, logm)))
    return cells


_built = {}


def build(shp):
    n, sizes, t, variance, batch = shp
    key = (n, tuple(sizes), t, variance)
    if key not in _built:   # (seconds at n = 16384, and two tests walk the matrix)
        _built[key] = obfv.BfvParameters(n, t, moduli_sizes=sizes, variance=variance)   # raises NonInvertible / NotEnoughPrimes
    opar = _built[key]
    assert opar.moduli_sizes == sizes and t % (2 * n) == 1 and t not in opar.moduli
    assert 1 <= variance <= 32 and batch >= 1
    return opar


def test_matrix_shapes_cover_every_instance():
    shapes = S.matrix_shapes()
    assert shapes == S.matrix_shapes()
    need = required_cells()
    assert len(need) == 7 * 33 == 231
    got = set()
    by_logm = {}
    for shp in shapes:
        opar = build(shp)
        mine = launched_cells(opar)
        assert mine == S.cells(shp), shp
        got |= mine
        by_logm.setdefault(opar.degree().bit_length() - 1, []).append(opar)
        if opar.degree() >= 4096:
            assert len(opar.moduli) in (2, 3)
    assert got == need, sorted(need - got)
    assert S.all_cells() == need
    # the mod-t words are reduced into narrower q_i at every tile size, and into every q_i of one shape
    for logm in range(3, 15):
        assert any(o.plaintext > min(o.moduli) for o in by_logm[logm]), logm
        assert any(o.plaintext > max(o.moduli) for o in by_logm[logm]), logm
    # t as wide as the general instances take, the stock 20 bits, and one of each F64 class
    widths = {o.plaintext.bit_length() for os_ in by_logm.values() for o in os_}
    assert {20, 48, 49, 50, 61} <= widths and any(51 <= w <= 59 for w in widths)


def test_mbfv_cells_cover_every_instance():
    """mbfv_share_kernel<LOGM, NARROW, F64, FORM>: the matrix case (mbfv_shape_cases.case_shape) launches MBFV_AX (0) and
    MBFV_AXX (1) over the moduli of level 0 and of the deepest level, MBFV_AX_WY (2, round-1 h0) over the level-0
    moduli; the union over the matrix is every one of the 33 x 3 instances."""
    need = {("mbfv_share_kernel", logm, k, form) for kern, logm, k in required_cells() if kern == "ksk_gen_kernel"
            for form in (0, 1, 2)}
    assert len(need) == 3 * 33 == 99 and S.MBFV_FORMS == (0, 1, 2)
    got = set()
    differ = 0
    for shp in S.matrix_shapes():
        opar = build(shp)
        assert len(opar.moduli) >= 2   # (the relin rounds run on every matrix shape)
        logm = opar.degree().bit_length() - 1
        k0, kd = kind(opar.ctx[0].moduli, logm), kind(opar.ctx[opar.max_level()].moduli, logm)
        differ += k0 != kd
        mine = {("mbfv_share_kernel", logm, k, form) for k in (k0, kd) for form in (0, 1)}
        mine.add(("mbfv_share_kernel", logm, k0, 2))
        assert mine == S.mbfv_cells(shp), shp
        got |= mine
    assert got == need == S.mbfv_all_cells(), sorted(need - got)
    assert differ   # (a deepest level of another kind than level 0's: [36, 62], [60, 52, 30], ...)
    # a single-modulus shape of the sweep runs no relin round
    assert {c[3] for c in S.mbfv_cells(S.shape(16, [62], 20, 10, 1))} == {0, 1}


def test_roundtrip_shapes_leave_room_for_fresh_noise():
    kinds = set()
    for shp in S.roundtrip_shapes():
        opar = build(shp)
        logm = opar.degree().bit_length() - 1
        assert sum(opar.moduli_sizes) - opar.plaintext.bit_length() >= 40
        kinds.add(kind(opar.moduli, logm))
        kinds.add("t%d" % opar.plaintext.bit_length())
        if opar.plaintext.bit_length() == 61:
            assert len(opar.plaintext_context.moduli) > 1
    assert {"general", "f64_3", "t61"} <= kinds


def test_random_shapes_are_accepted():
    seen_n, seen_v = set(), set()
    for idx in range(64):
        shp = S.random_shape(idx)
        assert shp == S.random_shape(idx)
        opar = build(shp)
        assert 8 <= opar.degree() <= 16384 and 1 <= len(opar.moduli) <= 4 and 1 <= shp[4] <= 5
        seen_n.add(opar.degree())
        seen_v.add(shp[3])
    assert {8, 16384} <= seen_n and seen_v == {1, 3, 10, 16, 17, 32}
