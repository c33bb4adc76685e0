"""CPU test: csrc/transcript.hpp compiled for the host -- the Keccak-f[1600], the byte sponge, the
tree digest, the six rounds of a proof, the batch weights and the circuit digest, which the
single-proof paths run on the host and the kernels of csrc/transcript.hip compile unchanged for the
device -- value by value against the pure-Python model tests/transcript_expect.py (itself checked
against hashlib in tests/test_transcript_expect.py)."""
import os
import random
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, HERE)

import transcript_expect as T  # noqa: E402

LENGTHS = [0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273]
COUNTS = [1, 2, 4, 5, 16, 17, 21]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("transcript_host")
    path = str(d / "transcript_host_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-w",
                    os.path.join(HERE, "native", "transcript_host_check.hip"), "-o", path], check=True)

    def go(lines):
        f = d / "in.txt"
        f.write_text("\n".join(lines) + "\n")
        out = subprocess.run([path, str(f)], capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out

    yield go
    shutil.rmtree(d, ignore_errors=True)


def h32(x):
    return "%064x" % x


def test_byte_sponge_at_block_edges_and_alignments(run):
    rng = random.Random(1)
    msgs = [(bytes(rng.randrange(256) for _ in range(n)), a) for n in LENGTHS for a in (0, 3)]
    out = run([f"keccak {len(m):x} {m.hex() or '-'} {a}" for m, a in msgs])
    assert out == [T.H(m).hex() for m, _ in msgs]


def test_tree_digest_shapes(run):
    rng = random.Random(2)
    cases = [(tag, [rng.randrange(T.R) for _ in range(m)]) for tag in (7, 8) for m in [0, 1, 3, 4, 5, 16, 17, 21, 65]]
    out = run([" ".join([f"tree {tag:x} {len(xs):x}"] + [h32(x) for x in xs]) for tag, xs in cases])
    assert out == [T.tree_digest(tag, [T.be32(x) for x in xs]).hex() for tag, xs in cases]


def _proof(rng, identity=None, big_field=None):
    pts = [(rng.randrange(1 << 254), rng.randrange(1 << 254)) for _ in range(9)]
    fs = [rng.randrange(T.R) for _ in range(7)]
    if identity is not None:
        pts[identity] = None
    if big_field is not None:
        fs[big_field] = (1 << 256) - 1 - rng.randrange(1 << 64)  # >= r: hashed as given
    return pts, fs


def _coords(pts):
    return [h32(c) for p in pts for c in (p or (0, 0))]


def test_proof_chain_and_batch_weights(run):
    rng = random.Random(3)
    h0 = bytes(rng.randrange(256) for _ in range(32))
    proofs = [_proof(rng) for _ in range(21)] + [_proof(rng, identity=3), _proof(rng, big_field=5)]
    pubs = [[rng.randrange(T.R) for _ in range(npub)] for npub in (0, 1, 4, 5, 17)]
    cases = [(pubs[i % 5], proofs[i]) for i in range(len(proofs))]
    out = run([" ".join([f"chain {h0.hex()} {len(pub):x}"] + [h32(x) for x in pub] + _coords(pts) + [h32(x) for x in fs])
               for pub, (pts, fs) in cases])
    t6s = []
    for line, (pub, (pts, fs)) in zip(out, cases):
        ch, t6 = T.proof_chain(h0, pub, pts, fs)
        assert line.split() == [h32(x) for x in T.chal5(ch)] + [h32(ch["u"]), t6.hex()]
        t6s.append(t6)
    out = run([" ".join([f"rho {c:x}"] + [t.hex() for t in t6s[:c]]) for c in COUNTS])
    assert [line.split() for line in out] == [[h32(x) for x in T.batch_rhos(t6s[:c])] for c in COUNTS]


def test_circuit_digest(run):
    rng = random.Random(4)
    pre = [(rng.randrange(1 << 254), rng.randrange(1 << 254)) for _ in range(7)] + [None]
    g2s = [rng.randrange(1 << 254) for _ in range(4)]
    cases = [(mode, n, npub, 2 + mode, 3 + n) for mode in (0, 1) for n, npub in ((8, 0), (1 << 20, 1024))]
    out = run([" ".join([f"circuit {m:x} {n:x} {k:x}", h32(k1), h32(k2)] + _coords(pre) + [h32(c) for c in g2s])
               for m, n, k, k1, k2 in cases])
    assert out == [T.circuit_digest(m, n, k, k1, k2, pre, g2s).hex() for m, n, k, k1, k2 in cases]
