"""A pure-Python model of the Fiat-Shamir transcript of the PLONK entry points (include/pbf.h
"Fiat-Shamir"): the Keccak sponge, the tree digest and the transcript, written from
the specification byte by byte -- no lanes, no limbs -- so it shares nothing with csrc/transcript.hpp
but the permutation's definition. tests/test_transcript_expect.py checks the sponge against
hashlib.sha3_256 (the same sponge with padding byte 0x06) and Ethereum's known answers."""

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MASK = (1 << 64) - 1
RATE = 136
DOMAIN = b"pbf-plonk-bn254-fiat-shamir-v1" + b"\0\0"
TAG_PUB, TAG_BATCH, TAG_RHO = 7, 8, 9


def _round_constants():
    """iota's constants from the degree-8 LFSR of the specification."""
    rcs, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) % 256
            if r & 2:
                rc |= 1 << ((1 << j) - 1)
        rcs.append(rc)
    return rcs


def _rotations():
    """rho's offsets: (t + 1)(t + 2) / 2 along the walk (x, y) -> (y, 2x + 3y)."""
    rot = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC = _round_constants()
ROT = _rotations()


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f(a):
    """Keccak-f[1600] on a[x][y], 5 x 5 lanes."""
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y], ROT[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & MASK & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def sponge256(msg, pad):
    """The 32-byte digest of the rate-136 sponge with first padding byte `pad` (0x01: Keccak-256,
    0x06: SHA3-256) and last padding bit 0x80."""
    msg = bytearray(msg)
    fill = RATE - len(msg) % RATE
    msg += bytes([pad]) + bytes(fill - 1)
    msg[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    for off in range(0, len(msg), RATE):
        for i in range(RATE // 8):
            a[i % 5][i // 5] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def H(msg):
    return sponge256(msg, 0x01)


def u64(k):
    return int(k).to_bytes(8, "big")


def be32(x):
    return int(x).to_bytes(32, "big")


def pt(p):
    """be32(x) | be32(y); the identity (None or (0, 0)) is 64 zero bytes."""
    return bytes(64) if p is None else be32(p[0]) + be32(p[1])


def challenge(digest):
    return int.from_bytes(digest, "big") % R


def tree_digest(tag, items):
    """items: 32-byte strings."""
    m = len(items)
    root = bytes(32)
    if m:
        while True:
            items = [H(b"".join(items[i:i + 4])) for i in range(0, len(items), 4)]
            if len(items) == 1:
                break
        root = items[0]
    return H(u64(tag) + u64(m) + root)


def circuit_digest(mode, n, npub, k1, k2, pre, g2s):
    """pre: the 8 preprocessed commitments q_m q_l q_r q_o q_c s_sigma_1..3; g2s: [s]G2 as the four
    coordinates of the entry points' 16 x u64 array, in its order."""
    assert len(pre) == 8 and len(g2s) == 4
    return H(DOMAIN + u64(mode) + u64(n) + u64(npub) + be32(k1) + be32(k2) + b"".join(pt(p) for p in pre)
             + b"".join(be32(c) for c in g2s))


def proof_chain(h0, pub, pts, fields):
    """pts: 9 points, fields: 7 ints (any 256-bit values, hashed as given). Returns
    {alpha, beta, gamma, z, v, u} and t6."""
    assert len(pts) == 9 and len(fields) == 7
    P = tree_digest(TAG_PUB, [be32(x) for x in pub])
    t1 = H(h0 + u64(1) + P + pt(pts[0]) + pt(pts[1]) + pt(pts[2]))
    t2 = H(t1 + u64(2))
    t3 = H(t2 + u64(3) + pt(pts[3]))
    t4 = H(t3 + u64(4) + pt(pts[4]) + pt(pts[5]) + pt(pts[6]))
    t5 = H(t4 + u64(5) + b"".join(be32(x) for x in fields))
    t6 = H(t5 + u64(6) + pt(pts[7]) + pt(pts[8]))
    ch = {"beta": challenge(t1), "gamma": challenge(t2), "alpha": challenge(t3), "z": challenge(t4),
          "v": challenge(t5), "u": challenge(t6)}
    return ch, t6


def chal5(ch):
    """alpha beta gamma z v: the order of the entry points' chal."""
    return [ch[k] for k in ("alpha", "beta", "gamma", "z", "v")]


def batch_rhos(t6s):
    T = tree_digest(TAG_BATCH, list(t6s))
    return [challenge(H(T + u64(TAG_RHO) + u64(i))) or 1 for i in range(len(t6s))]


def batch_challenges(h0, pubs, proofs):
    """([alpha beta gamma z v], [u], [rho]) of a batch; proofs: (pts, fields) pairs."""
    out = [proof_chain(h0, pub, pts, fs) for pub, (pts, fs) in zip(pubs, proofs)]
    return [chal5(c) for c, _ in out], [c["u"] for c, _ in out], batch_rhos([t for _, t in out])
