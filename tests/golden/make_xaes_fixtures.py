#!/usr/bin/env python3
"""Writes tests/golden/xaes256gcm_vectors.json: the two test vectors of the C2SP specification c2sp.org/XAES-256-GCM
(key, nonce, AAD, plaintext, the derived key Kx, ciphertext || tag) and the parameters of its accumulated test (10 000
iterations over the SHAKE-128 stream of the empty input; the digest of all outputs and the stream bytes consumed).  The
values are the specification's, typed in below; before anything is written every one of them is recomputed from the
oracle (tests/xaes_ref.py: encrypt_block cross-checked with cmac, then gcm_encrypt at 256 bits), so the file holds
nothing the composition does not reproduce.  Run by hand when the list changes; no test runs it.
Usage: make_xaes_fixtures.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NONCE = b"ABCDEFGHIJKLMNOPQRSTUVWX"
SPEC = [
    dict(key=b"\x01" * 32, nonce=NONCE, aad=b"", plaintext=b"XAES-256-GCM",
         kx="c8612c9ed53fe43e8e005b828a1631a0bbcb6ab2f46514ec4f439fcfd0fa969b",
         output="ce546ef63c9cc60765923609b33a9a1974e96e52daf2fcf7075e2271"),
    dict(key=b"\x03" * 32, nonce=NONCE, aad=b"c2sp.org/XAES-256-GCM", plaintext=b"XAES-256-GCM",
         kx="e9c621d4cdd9b11b00a6427ad7e559aeedd66b3857646677748f8ca796cb3fd8",
         output="986ec1832593df5443a179437fd083bf3fdb41abd740a21f71eb769d"),
]
ITERATIONS = 10000
DIGEST = "e6b9edf2df6cec60c8cbd864e2211b597fb69a529160cd040d56c0c210081939"


def main():
    path = os.path.join(HERE, "xaes256gcm_vectors.json")
    # the stream the accumulated test consumes: walked once here, so that the fixture can say how long it is
    s, pos = hashlib.shake_128(b"").digest(ITERATIONS * (32 + 24 + 2 + 510)), 0
    for _ in range(ITERATIONS):
        pos += 32 + 24
        pos += 1 + s[pos]
        pos += 1 + s[pos]
    vectors = [{k: (v.hex() if isinstance(v, bytes) else v) for k, v in vec.items()} for vec in SPEC]
    doc = dict(source="c2sp.org/XAES-256-GCM", vectors=vectors,
               accumulated=dict(iterations=ITERATIONS, stream_bytes=pos, digest=DIGEST))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    from tests import xaes_ref
    for v in xaes_ref.vectors():
        assert xaes_ref.derive(v["key"], v["nonce"]) == xaes_ref.derive_by_cmac(v["key"], v["nonce"]) == v["kx"]
        assert xaes_ref.encrypt(v["key"], v["nonce"], v["aad"], v["plaintext"]) == v["output"]
    got = xaes_ref.accumulated_digest(xaes_ref.encrypt(k, n, a, p) for k, n, p, a in xaes_ref.accumulated())
    assert got == DIGEST, got
    print(path, os.path.getsize(path), "bytes; stream", pos, "bytes; reference:", xaes_ref.check_vectors_through_the_reference())


if __name__ == "__main__":
    main()
