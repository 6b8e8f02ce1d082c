"""QUIC packet protection with AES-256-GCM on the GPU (a
SQOBFS_QUIC_AES_256_GCM keyring) against OpenSSL-built packets
(tests/golden/quic_gcm256.json), bit-exact: per-packet keys, one key from the
kernarg segment, the staged kernel of key-grouped batches, the fused
Salamander forms, and the rejects."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import sqobfs
from sqobfs import QuicKey

from test_gpu_quic import ctx, run  # noqa: F401  (fixture)
from test_gpu_quic_obfs import PSK, _open, _seal

pytestmark = pytest.mark.gpu
B = bytes.fromhex
S = sqobfs.QUIC_AES_256_GCM


@pytest.mark.parametrize("case,inplace,ungrouped", [
    ("packets", False, False), ("packets", True, False),  # 40 keys: per-packet entries (KM 1)
    ("key0", False, False), ("key0-ids", False, False),   # kernarg key (KM 0) / all-zero ids
    # the 64 stream records x 32 = 2,048 packets, 1,024 per key: the grouping
    # threshold; each key's 32 units = 2 full steps + 1 partial (KM 2)
    ("tiled", False, False), ("tiled", True, False), ("tiled", False, True),
    ("tiled", True, True)])
def test_seal_open_vs_openssl(ctx, golden, case, inplace, ungrouped):  # noqa: F811
    """Seal equals `protected`; open returns the packet, its length and pn."""
    f = golden("quic_gcm256.json")
    g = f["packets"] if case == "packets" else f["stream"] * 32 if case == "tiled" else \
        [v for v in f["stream"] if v["k"] == 0]
    keys = [QuicKey.of(B(v["key"]), B(v["iv"]), B(v["hp"]))
            for v in (g if case == "packets" else f["stream_keys"][:2 if case == "tiled" else 1])]
    kid = None if case == "key0" else np.array([v.get("k", i) for i, v in enumerate(g)])
    bad = set()
    if case == "tiled":  # ~1 % of the ids out of range
        bad = np.flatnonzero(np.random.Generator(np.random.PCG64(256)).random(len(g)) < 0.01)
        kid[bad] = 2 + bad % 3
        bad = set(bad.tolist())
    pkts, prot = [B(v["packet"]) for v in g], [B(v["protected"]) for v in g]
    pno = [v["pn_offset"] for v in g]
    sqobfs.debug_gcm_ungrouped(ungrouped)
    try:
        out, oo, ln, _, _ = run(ctx, keys, True, pkts, pno, [v["pn"] for v in g], key_ids=kid,
                                inplace=inplace, suite=S)
        out2, oo2, ln2, pn2, _ = run(ctx, keys, False, prot, pno, [v["largest_pn"] for v in g],
                                     key_ids=kid, inplace=inplace, suite=S)
    finally:
        sqobfs.debug_gcm_ungrouped(False)
    for i, v in enumerate(g):
        if i in bad:
            assert ln[i] == ln2[i] == sqobfs.QUIC_EKEY and pn2[i] == 0, i
            continue
        assert ln[i] == len(prot[i]) and ln2[i] == len(pkts[i]) and pn2[i] == v["pn"], i
        assert out[int(oo[i]):int(oo[i]) + ln[i]].tobytes() == prot[i], i
        assert out2[int(oo2[i]):int(oo2[i]) + ln2[i]].tobytes() == pkts[i], i


def test_fused_salamander(ctx, golden):  # noqa: F811
    f = golden("quic_gcm256.json")
    g, k = [v for v in f["stream"] if v["k"] == 0], f["stream_keys"][0]
    keys = [QuicKey.of(B(k["key"]), B(k["iv"]), B(k["hp"]))]
    pkts, pno = [B(v["packet"]) for v in g], [v["pn_offset"] for v in g]
    salts = [bytes([i, 7, 6, 5, 4, 3, 2, 1]) for i in range(len(g))]
    wires = []
    for v, s in zip(g, salts):
        key = np.frombuffer(hashlib.blake2b(PSK + s, digest_size=32).digest(), np.uint8)
        p = np.frombuffer(B(v["protected"]), np.uint8)
        wires.append(s + (p ^ np.resize(key, len(p))).tobytes())
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as kr_o:
        out, oo, ln, _ = _seal(ctx, keys, kr_o, pkts, pno, [v["pn"] for v in g], salts, suite=S)
        out2, oo2, ln2, pn2 = _open(ctx, keys, kr_o, wires, pno, [v["largest_pn"] for v in g],
                                    suite=S)
    for i, v in enumerate(g):
        assert ln[i] == len(wires[i]), i
        assert out[int(oo[i]):int(oo[i]) + ln[i]].tobytes() == wires[i], i
        assert ln2[i] == len(pkts[i]) and pn2[i] == v["pn"], i
        assert out2[int(oo2[i]):int(oo2[i]) + ln2[i]].tobytes() == pkts[i], i


def test_rejects(ctx, golden):  # noqa: F811
    f = golden("quic_gcm256.json")
    g, k = f["stream"][4:12], f["stream_keys"][0]  # key 0, payloads of 63 .. 4,000 B
    keys = [QuicKey.of(B(k["key"]), B(k["iv"]), B(k["hp"]))]
    bad = []
    for i, v in enumerate(g):  # one bit: in the tag (even i) or in the body, past the sample
        q = bytearray(B(v["protected"]))
        q[-1 - i if i % 2 == 0 else v["pn_offset"] + 24 + i] ^= 1 << (i % 8)
        bad.append(bytes(q))
    _, _, ln, _, _ = run(ctx, keys, False, bad, [v["pn_offset"] for v in g],
                         [v["largest_pn"] for v in g], suite=S)
    assert list(ln) == [sqobfs.QUIC_EAUTH] * len(g)
    with pytest.raises(sqobfs.SqError):
        sqobfs.QuicKeyring(ctx, keys, 3)
