"""FF3-1 (SP 800-38G revision 1) answers for tests/test_ff3_host.py and tests/test_gpu_ff3.py: the `Method = FF3-1`
stanzas of the reference's vector file (the withdrawn 64-bit-tweak FF3 is labelled `Method = FF3` and not selected), the
outputs the reference compiled with FF_X 3 gave (tests/golden/ff3_ref_vectors.json, recorded by
tests/golden/make_ff3_fixtures.py), and a plain-Python FF3-1 written from the specification, whose AES is the oracle's
ECB.  The chain of trust: vector file and recorded reference -> the model -> the engine's host path and the GPU."""
import json
import os

VECTOR_FILE = "FPE_FF1&FF3&FF3-1.tv"
FIXTURE_FILE = "ff3_ref_vectors.json"
DECIMAL = b"0123456789"
TWEAK = 7
ROUNDS = 8


def minlen(radix):
    n = 1
    while radix ** n < 1000000:
        n += 1
    return n


def maxlen(radix):
    """2 * floor(log_radix 2^96), exact integers"""
    k = 0
    while radix ** (k + 1) <= 1 << 96:
        k += 1
    return 2 * k


def _num(digits, radix):
    x = 0
    for d in digits:
        x = x * radix + d
    return x


def _str(x, radix, m):
    out = [0] * m
    for i in range(m - 1, -1, -1):
        x, out[i] = divmod(x, radix)
    return out


def model_batch(orc, key, tweaks, records, radix, decrypt=False):
    """FF3-1.Encrypt / FF3-1.Decrypt of SP 800-38G revision 1, algorithms 9 and 10, on equal-sized lists of digit
    values, record k under tweaks[k]; a round's cipher blocks of all records go to the oracle's ECB in one call"""
    rkey = bytes(key)[::-1]
    n = len(records[0])
    u = (n + 1) // 2
    v = n - u
    assert all(len(t) == TWEAK for t in tweaks) and all(len(r) == n for r in records) and len(tweaks) == len(records)
    tl = [bytes(t[0:3]) + bytes([t[3] & 0xF0]) for t in tweaks]
    tr = [bytes(t[4:7]) + bytes([(t[3] << 4) & 0xFF]) for t in tweaks]
    a = [list(r[:u]) for r in records]
    b = [list(r[u:]) for r in records]

    def f(i, ws, halves):
        ps = [w[:3] + bytes([w[3] ^ i]) + _num(h[::-1], radix).to_bytes(12, "big") for w, h in zip(ws, halves)]
        out = orc.ecb_encrypt(rkey, b"".join(p[::-1] for p in ps))
        return [int.from_bytes(out[16 * k:16 * k + 16][::-1], "big") for k in range(len(ps))]

    if not decrypt:
        for i in range(ROUNDS):
            m, ws = (u, tr) if i % 2 == 0 else (v, tl)
            c = [(_num(x[::-1], radix) + y) % radix ** m for x, y in zip(a, f(i, ws, b))]
            a, b = b, [_str(x, radix, m)[::-1] for x in c]
    else:
        for i in range(ROUNDS - 1, -1, -1):
            m, ws = (u, tr) if i % 2 == 0 else (v, tl)
            c = [(_num(x[::-1], radix) - y) % radix ** m for x, y in zip(b, f(i, ws, a))]
            b, a = a, [_str(x, radix, m)[::-1] for x in c]
    return [x + y for x, y in zip(a, b)]


def model(orc, key, tweak, digits, radix, decrypt=False):
    """the model on one list of digit values"""
    return model_batch(orc, key, [bytes(tweak)], [list(digits)], radix, decrypt)[0]


def model_text(orc, key, tweak, text, alphabet, decrypt=False):
    """the model on a byte string out of `alphabet`"""
    alphabet = bytes(alphabet)
    idx = {c: i for i, c in enumerate(alphabet)}
    out = model(orc, key, tweak, [idx[c] for c in bytes(text)], len(alphabet), decrypt)
    return bytes(alphabet[d] for d in out)


def vectors(golden_dir):
    """the FF3-1 stanzas of the reference's file: dicts of alphabet, key, tweak (7 bytes), pt, ct (bytes).  The ACVP
    samples carry an all-zero tweak written as eight bytes, which is the computation with seven zero bytes."""
    out, cur = [], {}
    with open(os.path.join(golden_dir, VECTOR_FILE), encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("#") or " = " not in line and not line.endswith(" ="):
                continue
            name, _, value = line.partition(" =")
            cur[name.strip()] = value.strip()
            if name.strip() == "CT":
                if cur.get("Method") == "FF3-1":
                    tweak = bytes.fromhex(cur["Tweak"])
                    if len(tweak) == 8:
                        assert tweak == bytes(8), cur
                        tweak = bytes(TWEAK)
                    assert len(tweak) == TWEAK, cur
                    out.append({"alphabet": cur["Alphabet"].encode(), "key": bytes.fromhex(cur["Key"]), "tweak": tweak,
                                "pt": cur["PT"].encode(), "ct": cur["CT"].encode()})
                cur = {}
    return out


def fixtures(golden_dir):
    """what the reference built with FF_X 3 gave: (entries, refusals).  An entry is a dict of key, tweak, pt, ct (bytes,
    decimal strings); a refusal a dict of key, tweak, text, prefill, encrypt_code / decrypt_code and the outputs left."""
    with open(os.path.join(golden_dir, FIXTURE_FILE)) as f:
        doc = json.load(f)
    entries = [{"key": bytes.fromhex(e["key"]), "tweak": bytes.fromhex(e["tweak"]), "pt": e["pt"].encode(),
                "ct": e["ct"].encode(), "what": e["what"]} for e in doc["entries"]]
    refusals = [{"key": bytes.fromhex(e["key"]), "tweak": bytes.fromhex(e["tweak"]), "text": bytes.fromhex(e["text"]),
                 "prefill": e["prefill"], "encrypt_code": e["encrypt_code"], "decrypt_code": e["decrypt_code"],
                 "encrypt_out": bytes.fromhex(e["encrypt_out"]), "decrypt_out": bytes.fromhex(e["decrypt_out"]),
                 "what": e["what"]} for e in doc["refusals"]]
    return entries, refusals
