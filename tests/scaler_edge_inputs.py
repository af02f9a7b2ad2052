"""Residue columns that put `RnsScaler::scale` (rns/scaler.rs:249-352) ON its rounding thresholds and walk its small
tables through their whole range -- inputs only, built from the oracle (never the engine); every expected value is
computed by the oracle where the columns are used (tests/test_scaler_edges.py, tests/scaler_edge_cases.py).

A random column leaves both fixed-point sums about 2^125 away from the value where the rounding flips, so a lost carry,
a dropped low partial product or `floor` for `ceil` changes no output word.  The classes here:

* `v_window`   x = (Q + 1) / 2 + delta: sum_i r_i theta_garner_i / 2^shift = v + x / Q up to the thetas' rounding, so v flips
               where x ~ Q / 2; delta uniform in +/-(4 Q >> (shift - 64)), at least +/-4.
* `v_lattice`  (five free source moduli of >= 50 bits) residues whose sum is at distance 0 ... 2 from a multiple of
               M = 2^(shift - 1), at both parities of the integer part: LLL + Babai rounding on the lattice with rows
               (e_i | W theta_i mod 2 M), (0 | W 2 M).  They depend on the source basis alone and take about a quarter
               of a second per basis, so they are built where they are used and no file of them is kept.
* `w_window`   the centred lift x_c with n' x_c = floor(d' / 2) + delta (mod d'), n' / d' the factor in lowest terms,
               |delta| <= d' >> 60 when d' > 2^61 (every fourth column at |delta| <= 1), else delta = 0 (for an even d'
               the exact tie).
* `w_lattice`  where v does not enter t (theta_gamma = 0: every t / Q scaler) the lattice again, over the signed theta_omega
               modulo 2^127: t within 0 ... 2 of an odd multiple of 2^126.
* `w_zero`     t ~ 0 from either side: x_c = 0, +/-1, +/-2 and n' x_c = +/-1 (mod d').
* `range`      r_i = floor(k (q_i - 1) / 64), k = 0 ... 64, on all sources, on the added terms of t alone and on the
               subtracted ones alone; each source alone at q_i - 1; all at q_i - 1 (attains the host's bounds).
"""
import random
from fractions import Fraction
from math import gcd

from fhe_oracle.rns import RnsContext, RnsScaler, ScalingFactor, M256
from fhe_oracle.zq import generate_prime

ROOT_ORDER = 512          # every modulus is 1 mod 512: usable at N = 16 and N = 256
SCALE_NFS = (3, 4, 5, 6, 8, 9, 10, 12, 14, 16, 17, 18, 20, 23, 27, 31, 33, 64)   # engine.hpp ScaleNFs
LATTICE_FREE = 5
LATTICE_LOWS = ("0", "1", "2", "M-1", "M-2")
N_WINDOW = 128


def scale_nf(nfrom):
    return min(nf for nf in SCALE_NFS if nf >= nfrom)


_primes = {}


def primes(bits, count, skip=()):
    """The `count` largest `bits`-bit primes that are 1 mod 512 and not in `skip`."""
    have = _primes.setdefault(bits, [])
    out = []
    i = 0
    while len(out) < count:
        if i == len(have):
            have.append(generate_prime(bits, ROOT_ORDER, have[-1] if have else 1 << bits))
        if have[i] not in skip:
            out.append(have[i])
        i += 1
    return out


def moduli_of(sizes, skip=()):
    """One prime per entry of `sizes` (bits), distinct, none from `skip`."""
    out = []
    for b in sizes:
        out.append(primes(b, 1, skip=tuple(skip) + tuple(out))[0])
    return out


class EdgeScaler:
    """One scaler under test: source and target moduli, the factor, and its oracle constants."""

    def __init__(self, name, frm, to, num, den, n=16):
        self.name, self.frm, self.to, self.num, self.den, self.n = name, list(frm), list(to), num, den, n
        self._rns = None

    @property
    def rns(self):
        if self._rns is None:
            self._rns = RnsScaler(RnsContext(self.frm), RnsContext(self.to), ScalingFactor(self.num, self.den))
        return self._rns

    @property
    def is_one(self):
        return self.num == self.den

    @property
    def ncommon(self):
        k = 0
        if self.is_one:
            while k < min(len(self.frm), len(self.to)) and self.frm[k] == self.to[k]:
                k += 1
        return k

    def __repr__(self):
        return "EdgeScaler(%s)" % self.name


# ---- the three bounds scaler_upload proves, restated (used to PICK sets and to assert branch cover, nothing else) ----------
def v_fits_64(sc):
    return sc.is_one and sum(q - 1 for q in sc.frm) + 2 < 1 << 64


def wide_w(sc):
    if sc.is_one:
        return False
    s = sc.rns
    bound = sum((lo | hi << 64) * (q - 1) for lo, hi, q in zip(s.theta_omega_lo, s.theta_omega_hi, sc.frm))
    bound += (s.theta_gamma_lo | s.theta_gamma_hi << 64) * (sum(q - 1 for q in sc.frm) + 2)
    return bound >= 1 << 191


def reduction_of(sc, j):
    """'narrow', 'fold' or 'general': the final reduction the kernel takes for target modulus j."""
    q = sc.to[j]
    k = q.bit_length()
    sum_q = sum(p - 1 for p in sc.frm)
    if sc.is_one and len(sc.to) <= 64 and (2 * sum_q + 2) * (q - 1) + 4 * q < 1 << (2 * k + 1):
        return "narrow"
    if len(sc.to) <= 64 and ((1 << 64) - 1 + sum_q) * (q - 1) + (1 << 65) + 4 * q < 1 << min(2 * k + 6, 128):
        return "fold"
    return "general"


def instance_of(sc):
    """(NF, kind) of the scale_kernel instance launch_scale picks."""
    nf = scale_nf(len(sc.frm))
    if v_fits_64(sc):
        return nf, "plain"
    return nf, "wide" if wide_w(sc) else "full"


# ---- the two sums and their distances from the thresholds -----------------------------------------------------------------
def v_sum(s, rests):
    return sum(r * (lo | hi << 64) for lo, hi, r in zip(s.theta_garner_lo, s.theta_garner_hi, rests)) & M256


def t_sum(s, rests, v=None):
    if v is None:
        v = s.scale_vw(rests)[0]
    t = 0
    for lo, hi, sg, r in zip(s.theta_omega_lo, s.theta_omega_hi, s.theta_omega_sign, rests):
        t += -(r * (lo | hi << 64)) if sg else r * (lo | hi << 64)
    g = v * (s.theta_gamma_lo | s.theta_gamma_hi << 64)
    return (t + g if s.theta_gamma_sign else t - g) & M256


def centred(x, m):
    x %= m
    return x - m if x > m // 2 else x


def v_distance(s, rests):
    """Distance of the v sum from the nearest value where ceil(. / 2) of its shifted form flips (an odd multiple of M)."""
    m = 1 << (s.theta_garner_shift - 1)
    return abs(centred(v_sum(s, rests) - m, 2 * m))


def v_boundary_distance(s, rests):
    """Distance of the v sum from the nearest multiple of M (where a bit leaves the shifted-out part)."""
    return abs(centred(v_sum(s, rests), 1 << (s.theta_garner_shift - 1)))


def v_outcome(s, rests):
    return (v_sum(s, rests) >> (s.theta_garner_shift - 1)) & 1


def t_signed(s, rests):
    t = t_sum(s, rests)
    return t - (1 << 256) if t >> 255 else t


def w_distance(s, rests):
    return abs(centred(t_sum(s, rests) - (1 << 126), 1 << 127))


def w_outcome(s, rests):
    t = t_sum(s, rests)
    if t >> 191:
        t = ~t & M256
    return (t >> 126) & 1


# ---- columns ------------------------------------------------------------------------------------------------------------------
def _rng(sc, tag):
    return random.Random("%s/%s" % (tag, ",".join(map(str, sc.frm))))


def project(x, moduli):
    return [x % q for q in moduli]


def v_window(sc, count=N_WINDOW):
    s, rng = sc.rns, _rng(sc, "v")
    big_q = s.frm.product
    span = max(4, (4 * big_q) >> (s.theta_garner_shift - 64))
    return [project((big_q + 1) // 2 + rng.randint(-span, span), sc.frm) for _ in range(count)]


def lowest_terms(sc):
    g = gcd(sc.num, sc.den)
    return sc.num // g, sc.den // g


def _centred_lifts(sc, residue, rng, count):
    """`count` centred lifts x_c (|x_c| < Q / 2) with n' x_c = residue (mod d')."""
    n1, d1 = lowest_terms(sc)
    big_q = sc.rns.frm.product
    x0 = centred(residue * pow(n1, -1, d1), d1) if d1 > 1 else 0
    kmax = (big_q // 2 - abs(x0)) // d1
    if kmax < 0:
        return []
    return [x0 + (rng.randint(-kmax, kmax) if kmax else 0) * d1 for _ in range(count if kmax else 1)]


def w_window(sc, count=N_WINDOW):
    """Window columns of w (d' > 2^61) or tie / nearest-to-tie columns (delta = 0)."""
    n1, d1 = lowest_terms(sc)
    if sc.is_one or d1 == 1:
        return []
    rng = _rng(sc, "w")
    span = d1 >> 60 if d1 > 1 << 61 else 0
    out = []
    for i in range(count):
        # (every fourth column at delta = -1, 0, 1: as near as the thetas' own rounding lets t come)
        delta = rng.randint(-span, span) if i % 4 else rng.randint(-1, 1) if span else 0
        out += _centred_lifts(sc, d1 // 2 + delta, rng, 1)
    return [project(x, sc.frm) for x in out]


def has_exact_tie(sc):
    n1, d1 = lowest_terms(sc)
    return not sc.is_one and d1 > 1 and d1 % 2 == 0


def w_zero(sc):
    n1, d1 = lowest_terms(sc)
    if sc.is_one:
        return []
    rng = _rng(sc, "z")
    xs = [0, 1, -1, 2, -2]
    if d1 > 1:
        for res in (1, -1):
            xs += _centred_lifts(sc, res, rng, 8)
    return [project(x, sc.frm) for x in xs]


def range_columns(sc):
    """-> {"all": [...65], "added": [...], "subtracted": [...], "single": [...], "max": [one]}"""
    s = sc.rns
    sign = s.theta_omega_sign
    walk = lambda keep: [[k * (q - 1) // 64 if keep(i) else 0 for i, q in enumerate(sc.frm)] for k in range(65)]
    out = {"all": walk(lambda i: True), "max": [[q - 1 for q in sc.frm]],
           "single": [[q - 1 if i == j else 0 for i, q in enumerate(sc.frm)] for j in range(len(sc.frm))]}
    if not sc.is_one:
        out["added"] = walk(lambda i: not sign[i])
        out["subtracted"] = walk(lambda i: sign[i])
    return out


# ---- lattice columns (v) ---------------------------------------------------------------------------------------------------
def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def lll(basis):
    """Textbook LLL (delta = 3/4) on integer rows, exact rational Gram-Schmidt."""
    b = [list(r) for r in basis]
    n = len(b)

    def gso():
        bs, mu, nrm = [], [[Fraction(0)] * n for _ in range(n)], []
        for i in range(n):
            v = [Fraction(x) for x in b[i]]
            for j in range(i):
                mu[i][j] = _dot(b[i], bs[j]) / nrm[j]
                v = [x - mu[i][j] * y for x, y in zip(v, bs[j])]
            bs.append(v)
            nrm.append(_dot(v, v))
        return mu, nrm

    mu, nrm = gso()
    k = 1
    while k < n:
        for j in range(k - 1, -1, -1):
            q = round(mu[k][j])
            if q:
                b[k] = [x - q * y for x, y in zip(b[k], b[j])]
                for l in range(j):
                    mu[k][l] -= q * mu[j][l]
                mu[k][j] -= q
        if nrm[k] >= (Fraction(3, 4) - mu[k][k - 1] ** 2) * nrm[k - 1]:
            k += 1
        else:
            b[k], b[k - 1] = b[k - 1], b[k]
            mu, nrm = gso()
            k = max(k - 1, 1)
    return b


def _inverse(rows):
    n = len(rows)
    a = [[Fraction(x) for x in r] + [Fraction(int(i == j)) for j in range(n)] for i, r in enumerate(rows)]
    for c in range(n):
        p = next(r for r in range(c, n) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [x / a[c][c] for x in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                a[r] = [x - a[r][c] * y for x, y in zip(a[r], a[c])]
    return [r[n:] for r in a]


def lattice_free_indices(frm):
    wide = [i for i, q in enumerate(frm) if q.bit_length() >= 50]
    return wide[:LATTICE_FREE] if len(wide) >= LATTICE_FREE else None


def lattice_targets(shift):
    """[(label, value mod 2 M)]: the five offsets from a multiple of M at an even and at an odd integer part."""
    m = 1 << (shift - 1)
    lows = dict(zip(LATTICE_LOWS, (0, 1, 2, m - 1, m - 2)))
    return [("%s/%s" % (low, par), lows[low] + p * m) for p, par in ((0, "even"), (1, "odd")) for low in LATTICE_LOWS]


def build_lattice_columns(frm, per_target=2):
    """Residue columns over `frm` whose v sum is (nearly) on each target of lattice_targets: five residues come from
    the lattice, the others are random and their part of the sum is folded into the target."""
    free = lattice_free_indices(frm)
    assert free is not None
    s = RnsScaler(RnsContext(frm), RnsContext([frm[0]]), ScalingFactor.one())
    shift = s.theta_garner_shift
    mod = 1 << shift
    theta = [lo | hi << 64 for lo, hi in zip(s.theta_garner_lo, s.theta_garner_hi)]
    return _babai_columns(frm, free, theta, mod, [v for _label, v in lattice_targets(shift)], per_target,
                          random.Random("lattice/" + ",".join(map(str, frm))))


def w_lattice_free_indices(sc):
    """The (at most five) widest sources with a non-zero theta_omega, where v does not enter t (theta_gamma = 0: the
    denominator divides numerator * Q, as in every t / Q scaler of BFV) and those sources leave room: 40 bits more than
    the 127 the target fixes."""
    if sc.is_one:
        return None
    s = sc.rns
    if s.theta_gamma_lo | s.theta_gamma_hi:
        return None
    live = [i for i in range(len(sc.frm)) if s.theta_omega_lo[i] | s.theta_omega_hi[i]]
    free = sorted(sorted(live, key=lambda i: -sc.frm[i])[:LATTICE_FREE])
    bits = sum(sc.frm[i].bit_length() for i in free)
    return free if len(free) >= 3 and bits >= 127 + 40 else None


W_LATTICE_LOWS = (0, 1, 2, -1, -2)


def w_lattice(sc, per_target=4):
    """Columns whose t is within a few units of an odd multiple of 2^126 (where w's rounding flips): the same lattice
    as for v, over the signed theta_omega of the free sources modulo 2^127."""
    free = w_lattice_free_indices(sc)
    if free is None:
        return []
    s = sc.rns
    mod = 1 << 127
    theta = [(-1 if sg else 1) * (lo | hi << 64) for lo, hi, sg in zip(s.theta_omega_lo, s.theta_omega_hi, s.theta_omega_sign)]
    return _babai_columns(sc.frm, free, theta, mod, [(1 << 126) + low for low in W_LATTICE_LOWS], per_target,
                          random.Random("wlattice/%s" % sc.name))


def _babai_columns(frm, free, theta, mod, values, per_target, rng):
    """Columns over `frm` with sum_i r_i theta_i = value (mod `mod`), as nearly as the lattice allows, for each value:
    the residues of `free` come from LLL + Babai rounding, the others are random and folded into the target."""
    weight = 1 << 40
    k = len(free)
    basis = [[int(i == j) for j in range(k)] + [weight * (theta[f] % mod)] for i, f in enumerate(free)]
    basis.append([0] * k + [weight * mod])
    red = lll(basis)
    inv = _inverse(red)
    cols = []
    for value in values:
        for _ in range(per_target):
            rests = [rng.randrange(q) for q in frm]
            rest_sum = sum(rests[i] * theta[i] for i in range(len(frm)) if i not in free)
            want = (value - rest_sum) % mod
            target = [rng.randrange(frm[f] // 4, 3 * frm[f] // 4) for f in free] + [weight * want]
            coef = [round(_dot(target, [inv[r][c] for r in range(k + 1)])) for c in range(k + 1)]
            point = [sum(coef[r] * red[r][c] for r in range(k + 1)) for c in range(k + 1)]
            for f, x in zip(free, point):
                assert 0 <= x < frm[f], "lattice residue out of range"
                rests[f] = x
            cols.append(rests)
    return cols


_lattice = {}


def lattice_columns(frm):
    """The lattice columns of a source basis (they depend on the basis alone: built once per process, about a quarter
    of a second each); [] where the basis has fewer than five moduli of >= 50 bits."""
    if lattice_free_indices(frm) is None:
        return []
    key = tuple(frm)
    if key not in _lattice:
        _lattice[key] = build_lattice_columns(frm)
    return [list(c) for c in _lattice[key]]


def classes(sc):
    """{class name: [columns]} for one scaler."""
    out = {"v_window": v_window(sc), "v_lattice": lattice_columns(sc.frm)}
    if not sc.is_one:
        out["w_window"] = w_window(sc)
        out["w_zero"] = w_zero(sc)
        out["w_lattice"] = w_lattice(sc)
    for name, cols in range_columns(sc).items():
        out["range_" + name] = cols
    return {k: v for k, v in out.items() if v}


THRESHOLD_CLASSES = ("v_lattice", "w_lattice", "v_window", "w_window", "w_zero")


# ---- the scalers --------------------------------------------------------------------------------------------------------------
TO3 = None


def _targets():
    """Targets of about 27, 50, 60 and 62 bits in one context (general, general, fold / general, narrow / fold / general)."""
    global TO3
    if TO3 is None:
        TO3 = [primes(27, 1)[0], primes(50, 1)[0], primes(60, 1)[0], primes(62, 1)[0]]
    return TO3


def plain_bits(nf):
    """The widest moduli at which nf of them keep sum (q_i - 1) + 2 below 2^64."""
    return 62 if nf <= 4 else 61 if nf <= 8 else 60 if nf <= 16 else 59 if nf <= 32 else 58


NON_UNIT = (3, 7)


def cell_scalers():
    """Every NF of ScaleNFs on its exact fit: factor one with v_fits_64 (PLAIN) and 3/7 (non-PLAIN, not WIDE_W: over
    narrower moduli where 3/7 over the PLAIN set would leave the fast path's range)."""
    out = []
    for nf in SCALE_NFS:
        frm = primes(plain_bits(nf), nf, skip=_targets())
        out.append(EdgeScaler("plain_nf%d" % nf, frm, _targets(), 1, 1))
        for bits in (plain_bits(nf), 56, 50):
            sc = EdgeScaler("full_nf%d_%db" % (nf, bits), primes(bits, nf, skip=_targets()), _targets(), *NON_UNIT)
            if not wide_w(sc):
                break
        out.append(sc)
    return out


def wide_threshold_count():
    """The smallest count of 62-bit source moduli at which 3/7 takes the WIDE_W instance."""
    for cnt in range(2, 41):
        if wide_w(EdgeScaler("", primes(62, cnt, skip=_targets()), _targets(), *NON_UNIT)):
            return cnt
    raise AssertionError("3/7 never wide")


def bound_scalers():
    """Source and target sets flanking each bound scaler_upload proves."""
    to = _targets()
    p62 = lambda c: primes(62, c, skip=to)
    out = [EdgeScaler("one_4x62", p62(4), to, 1, 1),                       # sum just below 2^64: v_fits_64
           EdgeScaler("one_5x62", p62(5), to, 1, 1),                       # above
           EdgeScaler("one_4x62_20", p62(4) + primes(20, 1), to, 1, 1),    # above by less than one (20-bit) modulus
           EdgeScaler("one_3x59", primes(59, 3, skip=to), to, 1, 1)]       # 62-bit target narrow, 60-bit fold
    cnt = wide_threshold_count()
    for c in sorted({cnt - 1, cnt, 24, 40}):
        out.append(EdgeScaler("w37_%dx62" % c, p62(c), to, *NON_UNIT))
    out.append(EdgeScaler("w23_24x62", p62(24), to, 2, 3))                 # t really passes 2^191 (3/7 over 24 does not)
    out.append(EdgeScaler("one_24x62", p62(24), to, 1, 1))                 # factor one, v >> 64 up to 2
    return out


DEFAULT_128 = {   # the reference's stock moduli (parameters.rs:222-251), as tests/ref_params.py holds them
    4096: [0xffffee001, 0xffffc4001, 0x1ffffe0001],
    8192: [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001],
}


def stock_plaintext(n):
    return generate_prime(20, 2 * n, (1 << 20) - 1)


def bfv_scalers():
    """The scalers of a ct x ct multiply and of a decryption at the stock n = 4096 / 8192 sets (rows of 16 columns)."""
    out = []
    for n, q in DEFAULT_128.items():
        t = stock_plaintext(n)
        ext, up = [], 1 << 62
        while len(ext) < -(-(sum(m.bit_length() for m in q) + 60) // 62):     # parameters.rs:660-676
            up = generate_prime(62, 2 * n, up)
            if up not in q:
                ext.append(up)
        big_q = 1
        for m in q:
            big_q *= m
        out.append(EdgeScaler("bfv%d_extend" % n, q, q + ext, 1, 1))
        out.append(EdgeScaler("bfv%d_down" % n, q + ext, q, t, big_q))
        acc = count = 0                                                        # parameters.rs:583-598
        while acc < t.bit_length() + 60 and count < len(q):
            acc += q[count].bit_length()
            count += 1
        out.append(EdgeScaler("bfv%d_decrypt" % n, q, q[:count], t, big_q))
    return out


GRID_Q3 = [4611686018282684417, 4611686018326724609, 4611686018309947393]     # tests/cases.py Q3, P3
GRID_P3 = [4611686018282684417, 4611686018309947393, 4611686018257518593]
GRID_NUMS = [1, 2, 3, 100, 1000, 4611686018326724610]
GRID_DENS = [1, 2, 3, 4, 100, 101, 1000, 1001, 4611686018326724610]


def grid_scalers():
    """The pairs of the scaler grid whose denominator stays even in lowest terms: they have an exact tie."""
    out = []
    for num in GRID_NUMS:
        for den in GRID_DENS:
            sc = EdgeScaler("grid_%d_%d" % (num, den), GRID_Q3, GRID_P3, num, den)
            if den % 2 == 0 and has_exact_tie(sc):
                out.append(sc)
    return out


def window_scalers():
    """The factors of the w window whose d' exceeds 2^61 (both rounding outcomes occur), on the sets it was measured on."""
    out = []
    for sizes in ([62, 62, 62], [50, 50, 40], [36, 62]):
        frm = moduli_of(sizes, skip=_targets())
        big_q = 1
        for m in frm:
            big_q *= m
        out.append(EdgeScaler("win_%s_1153_Q" % "_".join(map(str, sizes)), frm, _targets(), 1153, big_q))
        out.append(EdgeScaler("win_%s_1_2e62" % "_".join(map(str, sizes)), frm, _targets(), 1, 4611686018326724610))
    return out


_all = None


def all_scalers():
    global _all
    if _all is None:
        _all = cell_scalers() + bound_scalers() + bfv_scalers() + grid_scalers() + window_scalers()
        names = [s.name for s in _all]
        assert len(set(names)) == len(names)
    return _all


def lattice_bases():
    """The distinct source bases that get lattice columns."""
    seen = []
    for sc in all_scalers():
        if lattice_free_indices(sc.frm) is not None and sc.frm not in seen:
            seen.append(sc.frm)
    return seen
