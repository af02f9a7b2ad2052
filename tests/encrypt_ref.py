"""Test-side restatement of BFV encryption (crates/fhe-math/src/rq/mod.rs:298-330 `Poly::small`,
crates/fhe/src/bfv/keys/secret_key.rs:100-134 `encrypt_poly`, public_key.rs:47-97 `try_encrypt`), built from the
oracle's pieces: `seeded.ChaCha8Rng` (whose key is the seed itself, no hashing), `bfv.sample_vec_cbd` behind a
getrandbits(64) -> next_u64 adapter, `seeded.random_from_seed` and the Poly forms.  The transforms and pointwise
products run on the plain-C oracle so that full-size sets stay fast; `check_poly_forms` pins that path against the
pure-Python `Poly` at small sizes.

Shared by tests/test_encrypt_emu.py, tests/test_encrypt_gpu.py and tests/golden/make_encrypt_golden.py."""
import numpy as np

from fhe_oracle import bfv as obfv
from fhe_oracle import coracle
from fhe_oracle import seeded
from fhe_oracle.rq import Poly, NTT


class Bits:
    """sample_vec_cbd draws `rng.getrandbits(64)`: here that is the generator's next_u64."""

    def __init__(self, rng):
        self.rng = rng

    def getrandbits(self, k):
        assert k == 64
        return self.rng.next_u64()


def generator(seed):
    """ChaCha8Rng::from_seed(seed): the 32 seed bytes are the key."""
    return Bits(seeded.ChaCha8Rng(bytes(seed)))


def samples(seed, n, variance, draws=1):
    """`draws` consecutive sample_vec_cbd(n, variance) calls on one ChaCha8Rng::from_seed(seed)."""
    g = generator(seed)
    return [obfv.sample_vec_cbd(n, variance, g) for _ in range(draws)]


def lift(ctx, xs):
    """try_convert_from(&[i64], ctx, false): [L][N] residues."""
    return np.array([[x % q for x in xs] for q in ctx.moduli], dtype=np.uint64)


class Ring:
    """The plain-C oracle over one context (cached per context: building it costs a table copy)."""
    _cache = {}

    def __init__(self, ctx):
        self.ctx = ctx
        self.c = coracle.CCtx(ctx)

    @classmethod
    def of(cls, ctx):
        if id(ctx) not in cls._cache:
            cls._cache[id(ctx)] = cls(ctx)
        return cls._cache[id(ctx)]


def small(ctx, variance, seed, to_ntt=True):
    """Poly::small(ctx, variance, ChaCha8Rng::from_seed(seed)) -> [L][N]."""
    rows = lift(ctx, samples(seed, ctx.degree, variance)[0])
    return Ring.of(ctx).c.poly_ntt_forward(rows) if to_ntt else rows


def encrypt_sk(ctx, variance, s_ntt, a_seed, e_seed, pt=None):
    """SecretKey::encrypt_poly with a = random_from_seed(a_seed), e = small(e_seed): -> [2][L][N] Ntt."""
    r = Ring.of(ctx).c
    a = np.array(seeded.random_from_seed(ctx.moduli, ctx.degree, bytes(a_seed)), dtype=np.uint64)
    e = small(ctx, variance, e_seed)
    c0 = r.poly_sub(e, r.poly_mul(a, s_ntt))
    if pt is not None:
        c0 = r.poly_add(c0, pt)
    return np.stack([c0, a])


def encrypt_pk(ctx, variance, pk, seed, pt=None):
    """PublicKey::try_encrypt with u, e1, e2 three draws of ChaCha8Rng::from_seed(seed): -> [2][L][N] Ntt."""
    r = Ring.of(ctx).c
    u, e1, e2 = (r.poly_ntt_forward(lift(ctx, x)) for x in samples(seed, ctx.degree, variance, 3))
    c0 = r.poly_add(r.poly_mul(u, pk[0]), e1)
    if pt is not None:
        c0 = r.poly_add(c0, pt)
    c1 = r.poly_add(r.poly_mul(u, pk[1]), e2)
    return np.stack([c0, c1])


def secret_key(opar, seed):
    """The oracle's SecretKey whose coefficients are SecretKey::random's draw from ChaCha8Rng::from_seed(seed)."""
    return obfv.SecretKey(opar, samples(seed, opar.degree(), opar.variance)[0])


def check_poly_forms(opar, seed, level=0):
    """The C-oracle path above equals the pure-Python Poly forms: small (both representations) and encrypt_poly's
    c0 = e - a s + m."""
    ctx = opar.ctx[level]
    v = opar.variance
    xs = samples(seed, ctx.degree, v)[0]
    assert small(ctx, v, seed, False).tolist() == Poly.from_i64(ctx, xs).coefficients
    assert small(ctx, v, seed).tolist() == Poly.from_i64(ctx, xs, NTT).coefficients
    sk = secret_key(opar, bytes(reversed(seed)))
    s = Poly.from_i64(ctx, sk.coeffs, NTT)
    a = Poly(ctx, NTT, seeded.random_from_seed(ctx.moduli, ctx.degree, bytes(seed)))
    m = sk.encode_poly(list(range(ctx.degree)), level)
    want = Poly.from_i64(ctx, xs, NTT).sub(a.mul(s)).add(m)
    got = encrypt_sk(ctx, v, np.array(s.coefficients, dtype=np.uint64), seed, seed,
                     np.array(m.coefficients, dtype=np.uint64))
    assert got[0].tolist() == want.coefficients
    assert got[1].tolist() == a.coefficients
