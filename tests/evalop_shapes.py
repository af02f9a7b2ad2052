"""The kernel instances of the evaluation path -- ntt_kernel, ntt_global_kernel, tensor_intt_kernel, ks_fused_kernel,
ks_fused_split_kernel, ks_ntt_kernel, ks_mac_kernel -- as a table, the engine's dispatch rules restated in Python, and a
fixed list of shapes that reaches every instance a release build can launch.

A cell is (family, template arguments as the profiler prints them, run-time coordinates).  The tables follow the
dispatcher of csrc/engine.hpp (with_logn, with_row_kind, with_bool, with_tile, launch_ntt, launch_tensor_intt,
launch_ks_fused, launch_ks_ntt, key_switch_polys): rows larger than LDS run as 16384-point parts on the RNS loader
where the key's digits are residue rows, the F64 key switch at N = 4096 keeps 512 threads x 8, only N = 8192 runs the
resident item loop, and N = 16384 runs GM_MIXED (32) passes.

Row kinds, as in devop_shapes: general (a modulus >= 2^60), narrow (all below 2^60), and for whole rows of 4096 ... 16384
points the F64 classes 3 / 4 / 5 (widest modulus in [2^49, 2^50) / [2^48, 2^49) / below 2^48).

Three rules read the number of compute units: the tensor rule (a launch of at most one round of workgroups runs every
row on the general passes), two_per_cu (the 512-thread F64 key switch at N = 8192) and KS_AUTO.  Every shape forces its
key-switch mode, so KS_AUTO plays no part; matrix_shapes(cus) derives the batches of the other two from `cus`, and
cells(shape, cus) predicts what a shape launches.

Nothing here imports the engine."""
import functools
from collections import namedtuple

from fhe_oracle.bfv import extended_basis_primes, generate_moduli
from fhe_oracle.zq import generate_prime

import devop_shapes as DS

FAMILIES = ("ntt_kernel", "ntt_global_kernel", "tensor_intt_kernel", "ks_fused_kernel", "ks_fused_split_kernel",
            "ks_ntt_kernel", "ks_mac_kernel")
KS_GMAX, GM_MIXED = 3, 32          # kernels_passes.hpp
KS_FUSED, KS_UNFUSED, KS_UNFUSED_SUB, KS_FUSED_SUB = 1, 2, 3, 4   # engine.hpp (KS_AUTO = 0 is not under test)
LOGNS = range(3, 17)
TILES = range(3, 15)               # whole rows of one LDS tile
F64_TILES = range(12, 15)
HRS = (3, 4, 5)


def _a(*args):
    """Template arguments as the profiler's demangled symbol prints them."""
    return ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args)


# ---- the tables ---------------------------------------------------------------------------------------------------------
def _ntt_cells():
    out = set()
    for inv in (False, True):
        out |= {("ntt_kernel", _a(inv, lm, nrw, 1, False, 0)) for lm in TILES for nrw in (False, True)}
        out |= {("ntt_kernel", _a(inv, lm, False, 1, False, hr)) for lm in F64_TILES for hr in HRS}
    assert len(out) == 66
    gather = {("ntt_kernel", _a(True, lm, nrw, 1, True, 0)) for lm in F64_TILES for nrw in (False, True)}
    gather |= {("ntt_kernel", _a(True, lm, False, 1, True, hr)) for lm in F64_TILES for hr in HRS}
    assert len(gather) == 15
    return out | gather | {("ntt_kernel", _a(False, 13, True, 4, False, 0))}


def _tensor_cells():
    out = {("tensor_intt_kernel", _a(lm, False, nrw, 0)) for lm in TILES for nrw in (False, True)}
    out |= {("tensor_intt_kernel", _a(lm, False, False, hr)) for lm in F64_TILES for hr in HRS}
    assert len(out) == 33
    return out | {("tensor_intt_kernel", _a(13, True, nrw, 0)) for nrw in (False, True)}


def _ks_fused_cells():
    f = "ks_fused_kernel"
    out = {(f, _a(ln, nw, KS_GMAX, 0, False, 0, False, 0)) for ln in range(3, 12) for nw in (False, True)}
    assert len(out) == 18
    mid = {(f, _a(ln, nw, KS_GMAX, 0, rns, 0, gal, 0)) for ln in (12, 13) for nw in (False, True) for rns in (False, True)
           for gal in (False, True)}
    assert len(mid) == 16
    top = {(f, _a(14, nw, GM_MIXED, 0, False, 0, gal, 0)) for nw in (False, True) for gal in (False, True)}
    f64 = {(f, _a(ln, False, KS_GMAX, tt, True, 0, gal, hr)) for ln in F64_TILES for hr in HRS for gal in (False, True)
           for tt in ((0, 512) if ln == 13 else (0,))}
    assert len(f64) == 24
    parts = {(f, _a(14, nw, GM_MIXED, 0, rns, g0, gal, 0)) for g0 in (1, 2) for nw in (False, True) for rns in (False, True)
             for gal in (False, True)}
    assert len(parts) == 16
    return out | mid | top | f64 | parts


def _ks_ntt_cells():
    f = "ks_ntt_kernel"
    out = {(f, _a(lm, 0, nw, False, 0)) for lm in range(3, 12) for nw in (False, True)}
    out |= {(f, _a(lm, 0, nw, rns, 0)) for lm in F64_TILES for nw in (False, True) for rns in (False, True)}
    out |= {(f, _a(lm, 0, False, True, hr)) for lm in F64_TILES for hr in HRS}
    assert len(out) == 18 + 12 + 9
    sub = {(f, _a(13, g0, nw, rns, 0)) for g0 in (1, 2, 3) for nw in (False, True) for rns in (False, True)}
    return out | sub


REACHABLE = {
    "ntt_kernel": _ntt_cells(),
    "ntt_global_kernel": {("ntt_global_kernel", _a(inv, g0)) for inv in (False, True) for g0 in (2, 3)},
    "tensor_intt_kernel": _tensor_cells(),
    "ks_fused_kernel": _ks_fused_cells(),
    "ks_fused_split_kernel": {("ks_fused_split_kernel", _a(g0, 13, nw, rns)) for g0 in (2, 3) for nw in (False, True)
                              for rns in (False, True)},
    "ks_ntt_kernel": _ks_ntt_cells(),
    "ks_mac_kernel": {("ks_mac_kernel", "")},
}
COUNTS = {"ntt_kernel": 82, "ntt_global_kernel": 4, "tensor_intt_kernel": 35, "ks_fused_kernel": 78,
          "ks_fused_split_kernel": 8, "ks_ntt_kernel": 51, "ks_mac_kernel": 1}
assert {f: len(c) for f, c in REACHABLE.items()} == COUNTS and tuple(REACHABLE) == FAMILIES

# compiled, and called by no release path: {(family, args): reason}
UNREACHABLE = {}


def all_cells():
    return set().union(*REACHABLE.values())


assert len(all_cells()) == 259 and not UNREACHABLE


# ---- run-time coordinates ------------------------------------------------------------------------------------------------
# (family, args, (name, value)): what, beyond the symbol, a cell must have been run at
def required_coords():
    out = set()
    for nrw in (False, True):
        for logn in (13, 15, 16):
            out.add(("ntt_kernel", _a(True, 13, nrw, 1, False, 0), ("logn", logn)))
            out.add(("ntt_kernel", _a(True, 13, nrw, 1, True, 0), ("logn", logn)))
            out.add(("ntt_kernel", _a(False, 13, False, 1, False, 0), ("logn", logn)))
        for logn in (15, 16):
            out.add(("tensor_intt_kernel", _a(13, True, nrw, 0), ("logn", logn)))
            out.add(("ntt_kernel", _a(False, 13, True, 4, False, 0), ("logn", logn)))
    # the generic loaders (RNS = false, integer): lift modes 0 and 2 (Ksk::lift_mode), and a base-2^k decomposition key
    # where one is legal (single-modulus key contexts: no Galois fold is asked of them here, and no unfused form exists)
    for fam in ("ks_fused_kernel", "ks_fused_split_kernel", "ks_ntt_kernel"):
        for f, args in REACHABLE[fam]:
            a = args.split(", ")
            if a[4 if fam == "ks_fused_kernel" else 3] == "true":     # (the RNS argument)
                continue
            out |= {(f, args, ("lift", 0)), (f, args, ("lift", 2))}
            # (where no RNS instance exists -- below N = 4096, and the whole-row fused kernel at N = 16384 -- the generic
            # loader also takes the residue rows of same-width moduli, lift mode 1)
            if (fam == "ks_fused_kernel" and a[5] == "0" and not 12 <= int(a[0]) <= 13) or (fam == "ks_ntt_kernel" and int(a[0]) < 12):
                out.add((f, args, ("lift", 1)))
            if fam == "ks_fused_split_kernel" or (fam == "ks_fused_kernel" and a[6] == "false"):
                out.add((f, args, ("base", True)))
    out |= {("ks_mac_kernel", "", ("tile", t)) for t in ("n<512", "n=512", "n>512")}
    return out


# ---- the rules, restated -------------------------------------------------------------------------------------------------
def f64_class(moduli):
    """Ctx::f64_class over these moduli: 3 / 4 / 5, or 0 when one of them reaches 2^50."""
    widest = max(moduli)
    if widest >> 50:
        return 0
    return 3 if widest >> 49 else 4 if widest >> 48 else 5


def row_kind(moduli, lm, f64=True):
    """(narrow, hr) of a whole-row launch over `moduli` (with_row_kind picks hr first, then narrow)."""
    hr = f64_class(moduli) if f64 and lm in F64_TILES else 0
    return (False, hr) if hr else (max(moduli) < (1 << 60), 0)


def lift_mode(ct_moduli, ksk_moduli, log_base=0):
    """Ksk::lift_mode: 1 when a residue of any ciphertext modulus is below twice every key modulus, 2 below four times,
    else (and for base-2^k digits) 0."""
    if log_base:
        return 0
    mx, mn = max(ct_moduli), min(ksk_moduli)
    return 1 if mx < 2 * mn else 2 if mx < 4 * mn else 0


def ks_rns(moduli, log_base=0):
    return not log_base and lift_mode(moduli, moduli) == 1


def mul_basis(n, moduli):
    """The multiplication context of Multiplicator::default at level 0 (full_size.oracle_level)."""
    return list(_mul_basis(n, tuple(moduli)))


@functools.lru_cache(maxsize=None)
def _mul_basis(n, moduli):
    n_ext = -(-(sum(m.bit_length() for m in moduli) + 60) // 62)
    return list(moduli) + extended_basis_primes(n, list(moduli), n_ext)


def tensor_fills(l_ext, nb, lm, cus):
    """launch_tensor_intt's rule: the narrow / F64 instances run only when the launch is more than one round of
    workgroups (two a compute unit, one with 16384-point tiles); devices of at most 8 units always take them."""
    lsub = lm - 13 if lm > 14 else 0
    return cus <= 8 or ((3 * l_ext * nb) << lsub) > cus * (1 if lm == 14 else 2)


def tensor_batch(l_ext, lm, cus):
    """The smallest batch at which the tensor launch takes its narrow / F64 instances."""
    nb = 1
    while not tensor_fills(l_ext, nb, lm, cus):
        nb += 1
    return nb


def mac_tile(n):
    return "n<512" if n < 512 else "n=512" if n == 512 else "n>512"


# ---- shapes ----------------------------------------------------------------------------------------------------------------
# ops: "ntt" forward and inverse transforms; "mul" Multiplicator.multiply without a key; "ks" / "relin" / "rot"
# key_switch, relinearisation and one rotation (exponent 3) under a synthetic key with the mode forced; "ksb" key_switch
# under a base-2^k decomposition key (one modulus).  what: the reason the shape is in the matrix.
Shape = namedtuple("Shape", "n sizes batch mode ops moduli log_base what")


@functools.lru_cache(maxsize=None)
def _prime(bits, n, upper=None):
    p = generate_prime(bits, 2 * n, upper if upper is not None else 1 << bits)
    assert p is not None and p.bit_length() == bits, (bits, n, upper)
    return p


@functools.lru_cache(maxsize=None)
def moduli_for(kind, lift, n):
    """Two explicit primes of the wanted row kind whose ratio gives the wanted lift mode.  general: 62 bits with 62 / 61
    (just above 2^60) / 40 bits; narrow: 60 bits with 60 / 59 (just above 2^58) / 40 bits."""
    top = 62 if kind == "general" else 60
    if lift == 1:
        q = _generate_moduli((top, top), n)
    elif lift == 2:
        q = [_prime(top, n), _prime(top - 1, n, 5 << (top - 4))]
    else:
        q = [_prime(top, n), _prime(40, n)]
    return tuple(q)


@functools.lru_cache(maxsize=None)
def _generate_moduli(sizes, n):
    return tuple(generate_moduli(list(sizes), n))


_F64_LISTS = {"f64_3": DS._CLASS3, "f64_4": DS._CLASS4, "f64_5": DS._CLASS5}
_BATCHES = (2, 1, 3)


def _check(shape, kind, lift=None):
    """The import-time assertions: the primes give the row kind, the F64 class, lift_mode and ks_rns the shape is for."""
    lm = shape.n.bit_length() - 1
    q = shape.moduli
    assert len(set(q)) == len(q) and all((m - 1) % (2 * shape.n) == 0 for m in q), shape
    assert [m.bit_length() for m in q] == list(shape.sizes), shape
    if kind.startswith("f64"):
        assert lm in F64_TILES and f64_class(q) == int(kind[-1]) and DS.row_kind(q, lm) == kind, shape
    else:
        assert row_kind(q, lm) == (kind == "narrow", 0) and (max(q) >> 60 != 0) == (kind == "general"), shape
        if lm in F64_TILES:
            assert DS.row_kind(q, lm) == kind, shape
    if lift is not None:
        assert lift_mode(q, q, shape.log_base) == lift and ks_rns(q, shape.log_base) == (lift == 1), shape
    return shape


@functools.lru_cache(maxsize=None)
def matrix_shapes(cus):
    """The fixed list that reaches every cell of all_cells() and every coordinate of required_coords() on a device of
    `cus` compute units.  Per row size and row kind: transforms and a multiply of one pair; a multiply at the smallest
    batch that takes the narrow / F64 tensor instances; key switch, relinearisation and a rotation per lift mode and
    key-switch mode; a decomposition key per integer kind.  N = 8192 on F64 rows also relinearises and rotates just
    above one polynomial row per compute unit (the 512-thread instance)."""
    out = []

    def add(n, q, batch, mode, ops, what, kind, lift=None, log_base=0):
        out.append(_check(Shape(n, tuple(m.bit_length() for m in q), batch, mode, tuple(ops), tuple(q), log_base, what),
                          kind, lift))

    for lm in LOGNS:
        n = 1 << lm
        kinds = ("general", "narrow") + (tuple(_F64_LISTS) if lm in F64_TILES else ())
        modes = {14: (KS_FUSED, KS_UNFUSED, KS_UNFUSED_SUB), 15: (KS_FUSED, KS_UNFUSED, KS_FUSED_SUB),
                 16: (KS_FUSED, KS_UNFUSED, KS_FUSED_SUB)}.get(lm, (KS_FUSED, KS_UNFUSED))
        for kind in kinds:
            if kind.startswith("f64"):
                sets = [(None, _generate_moduli(tuple(_F64_LISTS[kind][lm % 3]), n))]
            else:
                sets = [(lift, moduli_for(kind, lift, n)) for lift in (0, 2, 1)]
            for lift, q in sets:
                # (sub-block tiles have no F64 instances: an F64 shape there would repeat a narrow one)
                for mode in (m for m in modes if not (kind.startswith("f64") and m == KS_UNFUSED_SUB)):
                    # (F64 rows at N = 8192: at most one polynomial row per compute unit here, whatever the device)
                    batch = 1 if kind.startswith("f64") and lm == 13 else _BATCHES[len(out) % 3]
                    add(n, q, batch, mode, ("ks", "relin", "rot"), "key switch", kind, lift)
            q = sets[-1][1]
            add(n, q, 1, KS_FUSED, ("ntt", "mul"), "transforms, one pair", kind)
            if kind != "general":
                nb = tensor_batch(len(mul_basis(n, q)), lm, cus)
                if nb > 1:
                    add(n, q, nb, KS_FUSED, ("mul",), "tensor launch of more than one round", kind)
            if kind.startswith("f64") and lm == 13:
                add(n, q, cus // len(q) + 1, KS_FUSED, ("relin", "rot"), "two workgroups per compute unit", kind)
            if not kind.startswith("f64"):
                q1 = [_prime(62 if kind == "general" else 60, n)]
                for mode in (KS_FUSED,) + ((KS_FUSED_SUB,) if lm > 14 else ()):
                    lb = (q1[0] - 1).bit_length() // 2
                    add(n, q1, _BATCHES[len(out) % 3], mode, ("ksb",), "decomposition key", kind, 0, lb)
    return tuple(out)


# the import-time assertions on the primes (they do not depend on the device)
assert len(matrix_shapes(256)) > 0


# ---- what a shape launches -------------------------------------------------------------------------------------------------
def _ntt_cells_of(q, lm, inverse, gather, f64):
    """launch_ntt over all rows of a context."""
    if lm <= 14:
        nrw, hr = row_kind(q, lm, f64)
        assert not gather or lm >= 12
        return {("ntt_kernel", _a(inverse, lm, nrw, 1, gather, hr), (("logn", lm),) if lm == 13 and not hr else ())}
    nrw = max(q) < (1 << 60)
    c = (("logn", lm),)
    out = {("ntt_global_kernel", _a(inverse, lm - 13), ())}
    if inverse:
        out.add(("ntt_kernel", _a(True, 13, nrw, 1, gather, 0), c))
    elif nrw:
        out.add(("ntt_kernel", _a(False, 13, True, 4, False, 0), c))
    else:
        out.add(("ntt_kernel", _a(False, 13, False, 1, False, 0), c))
    return out


def _tensor_cells_of(n, q, nb, cus, f64):
    lm = n.bit_length() - 1
    basis = mul_basis(n, q)
    allow = tensor_fills(len(basis), nb, lm, cus)

    def kind_of(m):
        if not allow:
            return 0
        return 2 if row_kind([m], lm, f64)[1] else 1 if m < (1 << 60) else 0

    out, r0 = set(), 0
    while r0 < len(basis):
        r1 = r0 + 1
        while r1 < len(basis) and kind_of(basis[r1]) == kind_of(basis[r0]):
            r1 += 1
        kd = kind_of(basis[r0])
        if lm > 14:
            out.add(("tensor_intt_kernel", _a(13, True, kd == 1, 0), (("logn", lm),)))
        else:
            out.add(("tensor_intt_kernel", _a(lm, False, kd == 1, f64_class(basis[r0:r1]) if kd == 2 else 0), ()))
        r0 = r1
    if lm > 14:
        out.add(("ntt_global_kernel", _a(True, lm - 13), ()))
    return out


def _ks_cells_of(shape, npolys, gal, cus, f64):
    """key_switch_polys with the mode forced (never KS_AUTO)."""
    n, q, mode, lb = shape.n, list(shape.moduli), shape.mode, shape.log_base
    lm = n.bit_length() - 1
    narrow, rns, lift = max(q) < (1 << 60), ks_rns(q, lb), lift_mode(q, q, lb)
    generic = (("base", True),) if lb else (("lift", lift),)     # the coordinate of an RNS = false instance
    assert not gal or lm >= 12
    if not lb and mode in (KS_UNFUSED, KS_UNFUSED_SUB):
        logm = 13 if lm > 14 or (lm == 14 and mode == KS_UNFUSED_SUB) else lm
        g0 = lm - logm
        hr = f64_class(q) if g0 == 0 and f64 and lm in F64_TILES else 0
        if hr:
            a = ("ks_ntt_kernel", _a(logm, 0, False, True, hr), ())
        else:
            r = rns and logm >= 12
            a = ("ks_ntt_kernel", _a(logm, g0, narrow, r, 0), () if r else generic)
        return {a, ("ks_mac_kernel", "", (("tile", mac_tile(n)),))}
    if lm <= 14:
        # (the F64 words exist when every key modulus is below 2^50 and the digits are residue rows)
        hr = f64_class(q) if f64 and not lb and lm in F64_TILES else 0
        if hr:
            tt = 512 if lm == 13 and npolys * len(q) > cus else 0
            return {("ks_fused_kernel", _a(lm, False, KS_GMAX, tt, True, 0, gal, hr), ())}
        r = rns and lm in (12, 13)
        return {("ks_fused_kernel", _a(lm, narrow, GM_MIXED if lm == 14 else KS_GMAX, 0, r, 0, gal, 0), () if r else generic)}
    if mode == KS_FUSED:     # 16384-point parts, one / two folded stages
        return {("ks_fused_kernel", _a(14, narrow, GM_MIXED, 0, rns, lm - 14, gal, 0), () if rns else generic)}
    assert mode == KS_FUSED_SUB
    return {("ks_fused_split_kernel", _a(lm - 13, 13, narrow, rns), () if rns else generic)}


def cells(shape, cus, f64=True):
    """The cells the cases of tests/evalop_cases.py launch for one shape on a device of `cus` compute units: a subset of
    what runs (the multiply's own transforms and scalers are not predicted), and all of it that the census counts on."""
    n, q = shape.n, list(shape.moduli)
    lm = n.bit_length() - 1
    out = set()
    for op in shape.ops:
        if op == "ntt":
            out |= _ntt_cells_of(q, lm, False, False, f64) | _ntt_cells_of(q, lm, True, False, f64)
        elif op == "mul":
            out |= _tensor_cells_of(n, q, shape.batch, cus, f64)
        elif op in ("ks", "ksb"):
            out |= _ks_cells_of(shape, shape.batch, False, cus, f64)
        elif op == "relin":     # the inverse transform of c2, then the key switch with both addends
            out |= _ntt_cells_of(q, lm, True, False, f64) | _ks_cells_of(shape, shape.batch, False, cus, f64)
        elif op == "rot":       # from N = 4096 the substitution is folded into the loaders
            fold = lm >= 12
            out |= _ntt_cells_of(q, lm, True, fold, f64) | _ks_cells_of(shape, shape.batch, fold, cus, f64)
        else:
            raise ValueError(op)
    assert {(f, a) for f, a, _c in out} <= all_cells(), out
    return out


def symbols_of(cell_set):
    return {(f, a) for f, a, _c in cell_set}


def coords_of(cell_set):
    return {(f, a, c) for f, a, cs in cell_set for c in cs}


def f64_eligible(shape):
    """One of the shape's launches takes an F64 instance while the switch is on (any device: the class of a row does
    not depend on the compute units)."""
    return symbols_of(cells(shape, 256, True)) != symbols_of(cells(shape, 256, False))


def coverage(cus):
    """(symbols, coordinates) the matrix reaches on a device of `cus` compute units under the restated rules."""
    sym, crd = set(), set()
    for s in matrix_shapes(cus):
        c = cells(s, cus)
        sym |= symbols_of(c)
        crd |= coords_of(c)
    return sym, crd


def census(launched_by_shape, shapes, cus):
    """(cells never launched, launched symbols outside the table, coordinates not covered) of a matrix run:
    launched_by_shape maps a shape's index to the (family, template arguments) its run launched.  A coordinate counts
    when a shape predicts it and that shape's run launched the cell's symbol."""
    seen = set().union(*launched_by_shape.values()) if launched_by_shape else set()
    coords = set()
    for i, launched in launched_by_shape.items():
        coords |= {(f, a, c) for f, a, c in coords_of(cells(shapes[i], cus)) if (f, a) in launched}
    return sorted(all_cells() - seen), sorted(seen - all_cells()), sorted(required_coords() - coords)
