"""GPU parity of the coset NTT / low-degree extension entry points (include/pbf.h
pbf_ntt_u64_coset*, pbf_ntt_fr256_coset*) against the oracle, bit for bit.

The expected values are built here from what the oracle already offers: a[j] * shift^j with
Python integers, zero padding, then oracle.ntt_iter (64-bit fields) or bn254.ntt (Fr); for the
inverse, the oracle's inverse followed by shift^-j. Sizes are the smallest that reach each
kernel shape: 2^3 and 2^12 the small kernel, 2^13 the smallest multi-pass Goldilocks plan
(passes 7,6), 2^16 (8,8), 2^18 (9,9), 2^20 (10,10: the 8192-element tiles), 2^21 (7,7,7)."""
import functools
import random

import numpy as np
import pytest

import bn254
import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
Q32 = 3221225473
R = bn254.R

EDGE_GL = [0, 1, 2, GOLD - 1, GOLD - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) - 1,
           GOLD - (1 << 32), GOLD - (1 << 32) + 1, (1 << 64) - (1 << 33), 0xFFFFFFFE00000001, 0x00000000FFFFFFFF,
           0x7FFFFFFF80000000]


def root(m, n):
    return pow(7 if m == GOLD else 5, (m - 1) // n, m)


def shift_of(m, which):
    """7, or a seeded random non-zero element"""
    return 7 if which == "7" else random.Random(0xC05E7 + m % 1000).randrange(2, m)


@functools.lru_cache(maxsize=4)
def powers(m, s, count):
    out, x = [], 1
    for _ in range(count):
        out.append(x)
        x = x * s % m
    return out


def scaled(m, a, s, n=None):
    """a[j] * s^j, zero-padded to n, as Python integers"""
    a = [int(x) for x in a]
    v = [x * p % m for x, p in zip(a, powers(m, s, len(a)))]
    return v + [0] * ((n or len(a)) - len(a))


def expect_fwd(m, w, s, a, n):
    return oracle.ntt_iter(m, w, np.array(scaled(m, a, s, n), dtype=np.uint64))


def expect_inv(m, w, s, f):
    inv = oracle.ntt_iter(m, w, f, inverse=True)
    return np.array(scaled(m, inv, pow(s, m - 2, m)), dtype=np.uint64)


def to_dev(host):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. forward and inverse against the oracle
CASES_1 = [(GOLD, l) for l in (3, 12, 13, 16, 18, 20, 21)] + [(Q32, l) for l in (3, 13, 16)]


@pytest.mark.parametrize("which", ["7", "random"])
@pytest.mark.parametrize("m,logn", CASES_1)
def test_coset_forward_inverse_vs_oracle(ctx, m, logn, which):
    n = 1 << logn
    in_len = n if logn < 21 else 1 << 19  # 2^21: a short input keeps the Python scaling cheap
    w, s = root(m, n), shift_of(m, which)
    a = oracle.splitmix_field(m, 4000 + logn, in_len)
    ref = expect_fwd(m, w, s, a, n)
    got = ctx.ntt_coset(m, w, s, a, n=n)
    assert np.array_equal(got, ref)
    back = ctx.ntt_coset(m, w, s, got, inverse=True)
    assert np.array_equal(back, expect_inv(m, w, s, ref))
    assert np.array_equal(back[:in_len], a) and not back[in_len:].any()  # the round trip, bit for bit


# ---- 2. prefixes (low-degree extension), batched, compact input
@pytest.mark.parametrize("frac", ["1", "n/4", "n/4+3", "n/2-1", "n-1"])
@pytest.mark.parametrize("logn", [13, 16, 20])
def test_coset_prefix_batch_dev(ctx, logn, frac):
    import torch

    n, batch, s = 1 << logn, 3, 7
    in_len = {"1": 1, "n/4": n // 4, "n/4+3": n // 4 + 3, "n/2-1": n // 2 - 1, "n-1": n - 1}[frac]
    w = root(GOLD, n)
    host = oracle.splitmix_field(GOLD, 4100 + logn, batch * in_len)
    d_in = to_dev(host)
    d_out = torch.empty(batch * n, dtype=torch.int64, device="cuda")
    ctx.ntt_coset_batch_dev(GOLD, w, s, d_in.data_ptr(), in_len, d_out.data_ptr(), n, batch,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = to_host(d_out)
    for b in range(batch):
        ref = expect_fwd(GOLD, w, s, host[b * in_len:(b + 1) * in_len], n)
        assert np.array_equal(out[b * n:(b + 1) * n], ref), b
    assert np.array_equal(to_host(d_in), host)  # the input is only read


# ---- 3. the two-stream group schedule: 9 polynomials = groups of 4, 4 and 1, on a non-default stream
def test_coset_group_schedule_side_stream(ctx):
    import torch

    n, batch, s = 1 << 13, 9, 7
    in_len = n // 4 + 3
    w = root(GOLD, n)
    host = oracle.splitmix_field(GOLD, 4200, batch * in_len)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = to_dev(host)
        d_out = torch.empty(batch * n, dtype=torch.int64, device="cuda")
        ctx.ntt_coset_batch_dev(GOLD, w, s, d_in.data_ptr(), in_len, d_out.data_ptr(), n, batch,
                                stream=side.cuda_stream)
        # in place (whole polynomials): the inverse of the evaluations, on the same stream
        ctx.ntt_coset_batch_dev(GOLD, w, s, d_out.data_ptr(), n, d_out.data_ptr(), n, batch, inverse=True,
                                stream=side.cuda_stream)
        d_fwd = torch.empty_like(d_out)
        ctx.ntt_coset_batch_dev(GOLD, w, s, d_out.data_ptr(), n, d_fwd.data_ptr(), n, batch, stream=side.cuda_stream)
    side.synchronize()
    back, fwd = to_host(d_out), to_host(d_fwd)
    for b in range(batch):
        a = host[b * in_len:(b + 1) * in_len]
        assert np.array_equal(fwd[b * n:(b + 1) * n], expect_fwd(GOLD, w, s, a, n)), b
        assert np.array_equal(back[b * n:b * n + in_len], a) and not back[b * n + in_len:(b + 1) * n].any(), b


# ---- 4. shift = 1 is the plain transform
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn", [13, 16, 20])
def test_coset_shift_one_is_plain(ctx, logn, inverse):
    n = 1 << logn
    w = root(GOLD, n)
    a = oracle.splitmix_field(GOLD, 4300 + logn, n)
    assert np.array_equal(ctx.ntt_coset(GOLD, w, 1, a, inverse=inverse), ctx.ntt(GOLD, w, a, inverse=inverse))
    if not inverse:  # and on a prefix: the plain transform of the zero-padded input
        pad = np.concatenate([a[:n // 4 + 3], np.zeros(n - n // 4 - 3, dtype=np.uint64)])
        assert np.array_equal(ctx.ntt_coset(GOLD, w, 1, a[:n // 4 + 3], n=n), ctx.ntt(GOLD, w, pad))


# ---- 5. edge values of the Goldilocks reduction, in the data and in the shift
@pytest.mark.parametrize("s", [GOLD - 1, 1 << 32, (1 << 32) - 1])
@pytest.mark.parametrize("logn", [13, 20])
def test_coset_edge_values(ctx, logn, s):
    n = 1 << logn
    w = root(GOLD, n)
    rng = np.random.default_rng(logn)
    a = np.array(EDGE_GL, dtype=np.uint64)[rng.integers(0, len(EDGE_GL), n)]
    ref = expect_fwd(GOLD, w, s, a, n)
    got = ctx.ntt_coset(GOLD, w, s, a)
    assert np.array_equal(got, ref)
    assert np.array_equal(ctx.ntt_coset(GOLD, w, s, a, inverse=True), expect_inv(GOLD, w, s, a))
    assert np.array_equal(ctx.ntt_coset(GOLD, w, s, got, inverse=True), a)


# ---- 6. the low-degree extension identity out[k] = a(shift * w^k)
def lde_samples(ctx, logn, in_len, seed):
    n, s = 1 << logn, 7
    w = root(GOLD, n)
    a = oracle.splitmix_field(GOLD, seed, in_len)
    got = ctx.ntt_coset(GOLD, w, s, a, n=n)
    ks = [0, 1, n // 2, n - 1] + [int(k) for k in np.random.default_rng(seed).integers(0, n, 12)]
    for k in ks:
        assert int(got[k]) == oracle.poly_eval(GOLD, a, s * pow(w, k, GOLD) % GOLD), k
    return w, s, a, got


def test_coset_lde_identity_2p16(ctx):
    lde_samples(ctx, 16, 1 << 14, 4400)


def test_coset_lde_identity_2p24(ctx):
    w, s, a, got = lde_samples(ctx, 24, 1 << 22, 4401)
    back = ctx.ntt_coset(GOLD, w, s, got, inverse=True)
    assert np.array_equal(back[:a.size], a) and not back[a.size:].any()


def regrouped_2p24_matches_stockham(ctx, w):
    import torch

    n, batch, s = 1 << 24, 2, shift_of(GOLD, "random")
    in_len = n // 4 + 3
    d_in = to_dev(oracle.splitmix_field(GOLD, 4402, batch * in_len))
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for c in (ctx, pbf.Context(0, options={"ntt.no_rg": "1"})):
        d_ev = torch.empty(batch * n, dtype=torch.int64, device="cuda")
        d_back = torch.empty_like(d_ev)
        c.ntt_coset_batch_dev(GOLD, w, s, d_in.data_ptr(), in_len, d_ev.data_ptr(), n, batch, stream=stream)
        c.ntt_coset_batch_dev(GOLD, w, s, d_ev.data_ptr(), n, d_back.data_ptr(), n, batch, inverse=True,
                              stream=stream)
        torch.cuda.synchronize()
        res.append((d_ev, d_back))
        if c is not ctx:
            c.close()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    back = to_host(res[0][1]).reshape(batch, n)
    assert np.array_equal(back[:, :in_len].reshape(-1), to_host(d_in)) and not back[:, in_len:].any()


def test_coset_regrouped_2p24_matches_stockham(ctx):
    """the regrouped 2^24 plan's coset variants (first / last pass) give the bits of the 8,8,8
    Stockham passes (context option ntt.no_rg), both directions, two polynomials"""
    regrouped_2p24_matches_stockham(ctx, root(GOLD, 1 << 24))


def test_coset_regrouped_2p24_inverse_root(ctx):
    """the same with the inverse root, whose forward transform runs the w_64 = 2^153 kernels and
    whose inverse the 2^39 ones: the regrouped coset first pass on 2^153 and last pass on 2^39"""
    regrouped_2p24_matches_stockham(ctx, pow(root(GOLD, 1 << 24), GOLD - 2, GOLD))


# ---- 7. argument errors, through the host entry points (they return before any launch)
def test_coset_errors(ctx):
    n = 16
    w = root(GOLD, n)
    a = list(range(1, n + 1))

    def einval(fn):
        with pytest.raises(pbf.PbfError) as e:
            fn()
        assert e.value.code == pbf.PBF_EINVAL

    einval(lambda: ctx.ntt_coset(GOLD, w, 0, a))
    einval(lambda: ctx.ntt_coset(GOLD, w, GOLD, a))
    einval(lambda: ctx.ntt_coset(Q32, root(Q32, n), Q32 + 5, a))
    einval(lambda: ctx.ntt_coset(GOLD, w, 7, [], n=n))
    einval(lambda: ctx.ntt_coset(GOLD, w, 7, a + [1], n=n))
    einval(lambda: ctx.ntt_coset(GOLD, w, 7, a[:5], n=n, inverse=True))
    einval(lambda: ctx.ntt_coset(GOLD, w, 7, [GOLD] + a[1:]))  # non-canonical input
    wf = bn254.root_of_unity(n)
    einval(lambda: ctx.ntt_fr_coset(wf, 0, a))
    einval(lambda: ctx.ntt_fr_coset(wf, R, a))
    einval(lambda: ctx.ntt_fr_coset(wf, 5, [], n=n))
    einval(lambda: ctx.ntt_fr_coset(wf, 5, a + [1], n=n))
    einval(lambda: ctx.ntt_fr_coset(wf, 5, a[:5], n=n, inverse=True))
    # and the context still works
    assert np.array_equal(ctx.ntt_coset(GOLD, w, 7, a), expect_fwd(GOLD, w, 7, a, n))


# ---- 8. BN254 Fr: the prover's scaling kernel and prefix transform behind the public entry points
@pytest.fixture(scope="module")
def ctx_l32():
    c = pbf.Context(0, options={"ntt256.l29": "0"})
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def fr_case(logn, short, s):
    n = 1 << logn
    in_len = n // 4 + 2 if short else n
    w = bn254.root_of_unity(n)
    a = bn254.limbs_to_ints(bn254.random_limbs(in_len, 4500 + logn))
    return w, a, bn254.ntt(scaled(R, a, s, n), w)


@pytest.mark.parametrize("l29", [True, False])
@pytest.mark.parametrize("s", [5, 2])
@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("logn", [3, 11, 13, 16])
def test_coset_fr(ctx, ctx_l32, logn, short, s, l29):
    c = ctx if l29 else ctx_l32
    n = 1 << logn
    w, a, ref = fr_case(logn, short, s)
    got = c.ntt_fr_coset(w, s, a, n=n)
    assert got == ref
    assert c.ntt_fr_coset(w, s, got, inverse=True) == a + [0] * (n - len(a))


def test_coset_fr_batch_dev_and_shift_one(ctx):
    import torch

    n, batch, s = 1 << 13, 3, 5
    in_len = n // 4 + 2
    w = bn254.root_of_unity(n)
    polys = [bn254.limbs_to_ints(bn254.random_limbs(in_len, 4600 + b)) for b in range(batch)]
    host = bn254.ints_to_limbs([x for p in polys for x in p])
    d_in = to_dev(host)
    d_out = torch.empty(batch * n * 4, dtype=torch.int64, device="cuda")
    ctx.ntt_fr_coset_batch_dev(w, s, d_in.data_ptr(), in_len, d_out.data_ptr(), n, batch,
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = bn254.limbs_to_ints(to_host(d_out))
    for b in range(batch):
        assert out[b * n:(b + 1) * n] == bn254.ntt(scaled(R, polys[b], s, n), w), b
    assert np.array_equal(to_host(d_in), host.reshape(-1))
    full = (polys[0] + polys[1] + polys[2] + polys[0])[:n]
    for inverse in (False, True):
        assert ctx.ntt_fr_coset(w, 1, full, inverse=inverse) == ctx.ntt_fr(w, full, inverse=inverse)


# ---- the other 64-bit paths and the table cache
def test_coset_size_one(ctx):
    for m in (GOLD, Q32):
        assert ctx.ntt_coset(m, 1, 7, [5]).tolist() == [5]
        assert ctx.ntt_coset(m, 1, 7, [5], inverse=True).tolist() == [5]
    assert ctx.ntt_fr_coset(1, 5, [9]) == [9]


@pytest.mark.parametrize("logn", [13, 16])
def test_coset_non_standard_root_generic_passes(ctx, logn):
    """w^3 has order n but w_64 is no power of two: the generic pass kernel with the scaling pass"""
    n, s = 1 << logn, 7
    w = pow(root(GOLD, n), 3, GOLD)
    a = oracle.splitmix_field(GOLD, 4700 + logn, n // 4 + 3)
    ref = expect_fwd(GOLD, w, s, a, n)
    got = ctx.ntt_coset(GOLD, w, s, a, n=n)
    assert np.array_equal(got, ref)
    assert np.array_equal(ctx.ntt_coset(GOLD, w, s, ref, inverse=True), expect_inv(GOLD, w, s, ref))


@pytest.mark.parametrize("logn", [13, 16])
def test_coset_two_level_factor_table(logn):
    """ntt.twmax_log below log2 n: the factor is a product of two table entries (the n > 2^24 path)"""
    c = pbf.Context(0, options={"ntt.twmax_log": "10"})
    n, s = 1 << logn, shift_of(GOLD, "random")
    w = root(GOLD, n)
    for in_len in (n // 4 + 3, n):
        a = oracle.splitmix_field(GOLD, 4800 + logn, in_len)
        ref = expect_fwd(GOLD, w, s, a, n)
        got = c.ntt_coset(GOLD, w, s, a, n=n)
        assert np.array_equal(got, ref)
    assert np.array_equal(c.ntt_coset(GOLD, w, s, ref, inverse=True), expect_inv(GOLD, w, s, ref))
    c.close()


def test_coset_table_cache_eviction(ctx):
    """more shifts than a plan keeps, a longer input after a shorter one, then the first again"""
    n = 1 << 13
    w = root(GOLD, n)
    a = oracle.splitmix_field(GOLD, 4900, n)
    shifts = [3, 5, 7, 11, 13, 17, 3]
    for i, s in enumerate(shifts):
        for in_len in (n // 4 + i, n):
            assert np.array_equal(ctx.ntt_coset(GOLD, w, s, a[:in_len], n=n), expect_fwd(GOLD, w, s, a[:in_len], n)), s


def test_coset_fft_trait_methods(ctx):
    n = 1 << 13
    ct = pbf.CooleyTurkey.new(GOLD, pbf.EvaluationDomainGenerator(root(GOLD, n), n), ctx)
    a = oracle.splitmix_field(GOLD, 5000, n // 4)
    ev = ct.coset_fft(a, 7, n=n)
    assert np.array_equal(ev, expect_fwd(GOLD, root(GOLD, n), 7, a, n))
    back = ct.coset_fft_inv(ev, 7)
    assert np.array_equal(back[:a.size], a) and not back[a.size:].any()
