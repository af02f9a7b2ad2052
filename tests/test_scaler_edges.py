"""The inputs of tests/scaler_edge_inputs.py, checked by the oracle alone (no engine): they sit where they claim to sit,
and every listed way of getting RnsScaler::scale (rns/scaler.rs:249-352) nearly right changes an output word on them --
so the engine tests on the same columns (tests/scaler_edge_cases.py) cannot pass vacuously.

Bounds asserted (from the construction, scaler_edge_inputs.py's docstring):
* window columns: both rounding outcomes on at least 25 % of the columns each, median distance of the sum from its
  threshold <= 2^70 (delta spans +/-4 Q >> (shift - 64), i.e. +/-2^66 in the sum; a random column is 2^125 away);
* lattice columns: distance <= 2^4 from the multiple of M aimed at (0, 1 or 2 by construction);
* exact ties (even d' <= 2^61): distance <= 2^70 (0 for d' = 2, 4; the thetas' rounding, < 2^66, otherwise)."""
import statistics

import pytest

import scaler_edge_inputs as I
from fhe_oracle.rns import RnsScaler, M128, M256

M64 = (1 << 64) - 1


def _by_name():
    return {s.name: s for s in I.all_scalers()}


def _names(pred=lambda s: True):
    return [s.name for s in I.all_scalers() if pred(s)]


@pytest.fixture(scope="module")
def scalers():
    return _by_name()


_classes = {}


def classes(sc):
    if sc.name not in _classes:
        _classes[sc.name] = I.classes(sc)
    return _classes[sc.name]


# ---- where the columns sit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names())
def test_v_window_straddles_the_threshold(scalers, name):
    sc = scalers[name]
    cols = classes(sc)["v_window"]
    up = sum(I.v_outcome(sc.rns, c) for c in cols)
    dist = [I.v_distance(sc.rns, c) for c in cols]
    print(name, "v window: up %d of %d, min 2^%d, median 2^%d" % (up, len(cols), min(dist).bit_length(),
                                                                  int(statistics.median(dist)).bit_length()))
    assert 4 * up >= len(cols) and 4 * (len(cols) - up) >= len(cols), (up, len(cols))
    assert statistics.median(dist) <= 1 << 70


@pytest.mark.parametrize("name", _names(lambda s: I.lattice_free_indices(s.frm) is not None))
def test_v_lattice_hits_its_targets(scalers, name):
    sc = scalers[name]
    cols = classes(sc)["v_lattice"]
    targets = [t for t in I.lattice_targets(sc.rns.theta_garner_shift) for _ in range(len(cols) // 10)]
    assert len(cols) == len(targets) == 20
    m = 1 << (sc.rns.theta_garner_shift - 1)
    worst = 0
    for (label, value), c in zip(targets, cols):
        assert all(0 <= r < q for r, q in zip(c, sc.frm))
        d = abs(I.centred(I.v_sum(sc.rns, c) - value, 2 * m))
        worst = max(worst, d)
        assert I.v_boundary_distance(sc.rns, c) <= 1 << 4, (label, d)
        if ((value + m // 2) // m) & 1:      # the multiple of M aimed at is odd: ceil(. / 2) flips there
            assert I.v_distance(sc.rns, c) <= 1 << 4, (label, d)
    print(name, "v lattice: worst distance from the target %d" % worst)
    assert worst <= 1 << 4
    assert {I.v_outcome(sc.rns, c) for c in cols} == {0, 1}     # both parities of the integer part


def _big_den(sc):
    return not sc.is_one and I.lowest_terms(sc)[1] > 1 << 61


@pytest.mark.parametrize("name", _names(_big_den))
def test_w_window_straddles_the_threshold(scalers, name):
    sc = scalers[name]
    cols = classes(sc)["w_window"]
    up = sum(I.w_outcome(sc.rns, c) for c in cols)
    dist = [I.w_distance(sc.rns, c) for c in cols]
    print(name, "w window: up %d of %d, min 2^%d, median 2^%d" % (up, len(cols), min(dist).bit_length(),
                                                                  int(statistics.median(dist)).bit_length()))
    assert 4 * up >= len(cols) and 4 * (len(cols) - up) >= len(cols), (up, len(cols))
    assert statistics.median(dist) <= 1 << 70


@pytest.mark.parametrize("name", _names(lambda s: I.has_exact_tie(s) and not _big_den(s)))
def test_w_ties_sit_on_the_threshold(scalers, name):
    sc = scalers[name]
    dist = [I.w_distance(sc.rns, c) for c in classes(sc)["w_window"]]
    print(name, "w ties: max 2^%d" % max(dist).bit_length())
    assert max(dist) <= 1 << 70
    if I.lowest_terms(sc)[1] in (2, 4):
        assert max(dist) == 0       # thetas are exact multiples of 2^125: t is ON the threshold


def allowed_signs(sc):
    """The signs t can take at all: a scaler whose non-zero terms are all added (or all subtracted) has a one-signed t."""
    s = sc.rns
    terms = [bool(sg) for lo, hi, sg in zip(s.theta_omega_lo, s.theta_omega_hi, s.theta_omega_sign) if lo | hi]
    if s.theta_gamma_lo | s.theta_gamma_hi:
        terms.append(not s.theta_gamma_sign)
    return set(terms)


@pytest.mark.parametrize("name", _names(lambda s: not s.is_one))
def test_t_near_zero_and_every_sign(scalers, name):
    """t = 0 exactly on the zero column, t at every sign its terms allow (`w_sign`: the reference's bit test), and for a
    wide denominator t within 2^70 of a multiple of 2^127 (of zero itself where the integer part is in v's term)."""
    sc = scalers[name]
    cl = classes(sc)
    assert I.t_sum(sc.rns, cl["w_zero"][0]) == 0
    signs = {sc.rns.scale_vw(c)[2] for cols in cl.values() for c in cols if any(c)}
    assert signs == allowed_signs(sc), (signs, allowed_signs(sc))
    n1, d1 = I.lowest_terms(sc)
    if d1 > 1 << 61:   # n' x_c = +/-1 (mod d'): |t| ~ 2^127 / d'
        near = [abs(I.centred(I.t_sum(sc.rns, c), 1 << 127)) for c in cl["w_zero"][1:]]
        assert min(near) <= 1 << 70, min(near).bit_length()


def test_both_signs_on_every_kind_of_instance(scalers):
    for kind in ("full", "wide"):
        assert any(allowed_signs(sc) == {False, True} for sc in scalers.values() if I.instance_of(sc)[1] == kind)


# ---- the tables' ranges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(lambda s: not I.v_fits_64(s)))
def test_every_high_word_of_v(scalers, name):
    """Every value of v >> 64 from 0 to the all-(q_i - 1) column's (the sum is monotone in each residue)."""
    sc = scalers[name]
    cl = classes(sc)
    top = sc.rns.scale_vw(cl["range_max"][0])[0] >> 64
    seen = {sc.rns.scale_vw(c)[0] >> 64 for c in cl["range_all"]}
    print(name, "v >> 64 up to", top)
    assert top < 16 and seen == set(range(top + 1)), (top, sorted(seen))


@pytest.mark.parametrize("name", _names(lambda s: not s.is_one))
def test_every_high_word_of_w(scalers, name):
    """|w| >> 64 over all columns.  Off the WIDE_W sets |t| < 2^191 (the bound scaler_upload proves), so |w| < 2^64 and
    its high word is 0 on every column -- the one value reachable; on the WIDE_W sets the positive w's high words have no
    gap from 0 to what the added-terms walk reaches."""
    sc = scalers[name]
    seen = set()
    for cols in classes(sc).values():
        for c in cols:
            _v, w, sign = sc.rns.scale_vw(c)
            if not sign:
                seen.add(w >> 64)
            elif not I.wide_w(sc):
                assert w >> 64 == 0
    print(name, "w >> 64 up to", max(seen, default=0))
    assert seen <= set(range(max(seen, default=0) + 1)) and (I.wide_w(sc) or seen <= {0})
    if seen:
        assert seen == set(range(max(seen) + 1)), sorted(seen)


def test_the_tables_are_walked_past_their_first_entry(scalers):
    """Some scaler reaches v >> 64 = 5: vhi_tab is read beyond entry 0 (w_tab's other entries are unreachable, above)."""
    vtop = max(sc.rns.scale_vw(classes(sc)["range_max"][0])[0] >> 64 for sc in scalers.values())
    assert vtop >= 5, vtop


def test_grid_is_the_scaler_grid():
    """The moduli and factors of the tie scalers are those of cases.case_scaler_grid."""
    import cases
    assert (I.GRID_Q3, I.GRID_P3, I.GRID_NUMS, I.GRID_DENS) == (cases.Q3, cases.P3, cases.NUMS, cases.DENS)
    assert len(I.grid_scalers()) == 17 and all(I.has_exact_tie(s) for s in I.grid_scalers())
    import ref_params
    assert all(I.DEFAULT_128[n] == ref_params.DEFAULT_128[n] for n in I.DEFAULT_128)
    assert all(I.stock_plaintext(n) == ref_params.plaintext_modulus(n) for n in I.DEFAULT_128)


def test_each_bound_is_flanked(scalers):
    """The sets picked from the restated bounds of scaler_upload lie where they were meant to."""
    s = scalers
    assert I.v_fits_64(s["one_4x62"]) and not I.v_fits_64(s["one_5x62"]) and not I.v_fits_64(s["one_4x62_20"])
    assert sum(q - 1 for q in s["one_4x62_20"].frm) + 2 - (1 << 64) < s["one_4x62_20"].frm[-1]     # within one modulus
    assert (1 << 64) - (sum(q - 1 for q in s["one_4x62"].frm) + 2) < 1 << 27
    cnt = I.wide_threshold_count()
    assert I.wide_w(s["w37_%dx62" % cnt]) and not I.wide_w(s["w37_%dx62" % (cnt - 1)])
    kinds = {I.reduction_of(sc, j) for sc in s.values() for j in range(sc.ncommon, len(sc.to))}
    assert kinds == {"narrow", "fold", "general"}
    one = s["one_3x59"]
    assert [I.reduction_of(one, j) for j in range(4)] == ["general", "general", "fold", "narrow"]
    assert [q.bit_length() for q in one.to] == [27, 50, 60, 62]
    cells = {I.instance_of(sc) for sc in s.values()}
    assert cells >= {(nf, k) for nf in I.SCALE_NFS for k in ("plain", "full")}
    assert {c for c in cells if c[1] == "wide"} == set(WIDE_CELLS)


WIDE_CELLS = [(6, "wide"), (27, "wide"), (64, "wide")]    # 3/7 over 6, 24 and 40 moduli of 62 bits (5 stay on the fast path)


# ---- mutants ------------------------------------------------------------------------------------------------------------------
class Mutant:
    """RnsScaler.scale with one step of scale_vw restated wrongly; everything else is the oracle's."""

    def __init__(self, s, kind):
        self._s, self.kind = s, kind

    def __getattr__(self, name):
        return getattr(self._s, name)

    def scale(self, rests, size, starting_index=0):
        return RnsScaler.scale(self, rests, size, starting_index)

    def scale_vw(self, rests):
        s, kind = self._s, self.kind
        vdrop = {"v_drop64": 64, "v_drop32": 32}.get(kind, 0)
        tdrop = {"t_drop64": 64, "t_drop32": 32}.get(kind, 0)
        acc = 0
        for lo, hi, ri in zip(s.theta_garner_lo, s.theta_garner_hi, rests):
            acc = (acc + (ri * (lo | (hi << 64)) >> vdrop << vdrop)) & M256
        acc >>= s.theta_garner_shift - 1
        v = (acc & M128) // 2 if kind == "v_floor" else ((acc & M128) + 1) // 2
        if kind == "v_mask64":
            v &= M64
        w_sign, w = False, 0
        if not s.scaling_factor.is_one:
            t = 0
            for lo, hi, sg, ri in zip(s.theta_omega_lo, s.theta_omega_hi, s.theta_omega_sign, rests):
                product = (ri * (lo | (hi << 64)) >> tdrop << tdrop) & M256
                t = (t - product) & M256 if sg else (t + product) & M256
            vtg = (v * (s.theta_gamma_lo | (s.theta_gamma_hi << 64)) >> tdrop << tdrop) & M256
            t = (t + vtg) & M256 if s.theta_gamma_sign else (t - vtg) & M256
            w_sign = (t >> 255) > 0 if kind == "sign_bit255" else (t >> 191) > 0
            if w_sign:
                # "neg_as_pos": the magnitude -t rounded like a positive t, for the reference's (~t >> 126) + 1 >> 1
                x = (-t & M256) if kind == "neg_as_pos" else (~t & M256)
                w = ((x >> 126) & M128) // 2 if kind == "w_floor" else (((x >> 126) & M128) + 1) // 2
            else:
                w = (t >> 126) & M128
                w = w // 2 if kind == "w_floor" else (w + 1) // 2
            if kind == "w_mask64":
                w &= M64
        return v, w, w_sign


def _caught(sc, kind, cols):
    s, m = sc.rns, Mutant(sc.rns, kind)
    size = len(sc.to) - sc.ncommon
    return sum(s.scale(c, size, sc.ncommon) != m.scale(c, size, sc.ncommon) for c in cols)


def _theta_gamma_zero(s):
    return not s.is_one and (s.rns.theta_gamma_lo | s.rns.theta_gamma_hi) == 0


# the WIDE_W sets whose t really passes 2^191 on the added-terms walk (the bound of scaler_upload adds the magnitudes of both
# signs, so 3/7 over 6 and over 24 moduli take the instance without leaving the fast path's range)
OUT_OF_RANGE = ("w37_40x62", "w23_24x62")


def test_t_leaves_the_fast_range_on_the_wide_sets(scalers):
    """On those sets columns exist with 2^191 <= t < 2^255: the reference calls them negative (`t >> 191 > 0`)."""
    for name in OUT_OF_RANGE:
        sc = scalers[name]
        assert I.instance_of(sc)[1] == "wide"
        n = sum(1 for c in classes(sc)["range_added"] if sc.rns.scale_vw(c)[2] and I.t_signed(sc.rns, c) > 0)
        print(name, "t in [2^191, 2^255) on %d of 65 columns" % n)
        assert n >= 1


# mutant -> (the scalers it applies to, the classes of theirs that must catch it)
MUTANTS = {
    "v_drop64": (lambda s: True, ("v_window", "v_lattice")),
    "v_drop32": (lambda s: True, ("v_lattice",)),
    "t_drop64": (lambda s: _big_den(s) or _theta_gamma_zero(s), ("w_window",)),
    "t_drop32": (lambda s: "w_lattice" in I.classes(s), ("w_lattice",)),
    "v_floor": (lambda s: True, ("v_window", "v_lattice")),
    "w_floor": (lambda s: _big_den(s) or I.has_exact_tie(s), ("w_window",)),
    "v_mask64": (lambda s: s.name in ("w37_24x62", "w37_40x62", "one_24x62"), ("range_all",)),
    "w_mask64": (lambda s: s.name in OUT_OF_RANGE, ("range_added",)),
    "sign_bit255": (lambda s: s.name in OUT_OF_RANGE, ("range_added",)),
    "neg_as_pos": (lambda s: I.lowest_terms(s)[1] == 2, ("w_window", "range_subtracted")),
}


@pytest.mark.parametrize("kind", sorted(MUTANTS))
def test_mutant_is_caught(scalers, kind):
    applies, cls = MUTANTS[kind]
    ran = 0
    for sc in scalers.values():
        if not applies(sc):
            continue
        for k in cls:
            cols = classes(sc).get(k)
            if cols:
                n = _caught(sc, kind, cols)
                ran += 1
                print("%s on %s / %s: %d of %d columns differ" % (kind, sc.name, k, n, len(cols)))
                assert n >= 1, (kind, sc.name, k)
    assert ran >= 1, "mutant %s met no class" % kind
