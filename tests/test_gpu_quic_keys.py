"""QUIC key update on the GPU: keyrings derived and rolled on the device from
TLS traffic secrets (sqobfs_quic_keyring_create_secrets / _rekey) and the
Key Phase resolver (sqobfs_quic_key_phase).  The references are HKDF from
hmac / hashlib and the host-built keyrings (pinned to OpenSSL by
test_gpu_quic_gcm*.py): a derived keyring must seal bit-identically to a host
keyring made from the HKDF keys."""
from __future__ import annotations

import hashlib
import hmac
import json
import struct

import numpy as np
import pytest
import sqobfs
from sqobfs import QuicKey, QuicKeyring, QuicSecret

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
B = bytes.fromhex
# suite, hash, key length
SUITES = [(sqobfs.QUIC_CHACHA20_POLY1305, hashlib.sha256, 32),
          (sqobfs.QUIC_AES_128_GCM, hashlib.sha256, 16),
          (sqobfs.QUIC_AES_256_GCM, hashlib.sha384, 32)]
PNO = 9  # short header: first byte, 8-byte connection id, 4-byte packet number


def expand_label(h, secret, label, n):
    info = struct.pack(">HB", n, 6 + len(label)) + b"tls13 " + label + b"\0"
    return hmac.new(secret, info + b"\x01", h).digest()[:n]  # n <= hash length: T(1)


def gen_key(h, kl, secret0, g):
    """The QuicKey of generation g: key and iv from the g-th "quic ku"
    successor of secret0, hp from secret0."""
    s = secret0
    for _ in range(g):
        s = expand_label(h, s, b"quic ku", h().digest_size)
    return QuicKey.of(expand_label(h, s, b"quic key", kl), expand_label(h, s, b"quic iv", 12),
                      expand_label(h, secret0, b"quic hp", kl))


def packet(rng, payload, pn, phase=0, first=0x43):
    return bytes([first | (phase << 2)]) + rng.bytes(8) + struct.pack(">I", pn & 0xFFFFFFFF) + \
        rng.bytes(payload)


def launch(ctx, fn, kr, pkts, pns, kid, pno=PNO):
    """One batch on the context's stream, out apart from in at the same
    offsets; returns (batch, device arrays, outputs cut to out_len < 2^20)."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)  # noqa: E731
    lens = np.array([len(p) for p in pkts], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens + 16 + 5)]).astype(np.uint64)
    data = np.zeros(int(off[-1]), np.uint8)
    for o, p in zip(off, pkts):
        data[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    d = dict(in_=t(data, np.uint8), off=t(off[:-1], np.uint64), len=t(lens, np.uint32),
             out=t(np.zeros_like(data), np.uint8), out_len=t(np.zeros(len(pkts)), np.uint32),
             pno=t(np.full(len(pkts), pno), np.uint16), pn=t(pns, np.uint64),
             kid=None if kid is None else t(kid, np.uint16),
             pn_out=t(np.zeros(len(pkts)), np.uint64))
    b = sqobfs.quic_batch(len(pkts), d["in_"], d["off"], d["len"], d["out"], d["off"],
                          d["out_len"], d["pno"], d["pn"], d["kid"], d["pn_out"])
    torch.cuda.synchronize(dev)
    if fn is not None:
        fn(ctx, kr, b)
        ctx.sync()
    out, ol_ = d["out"].cpu().numpy(), d["out_len"].cpu().numpy()
    return b, d, [out[int(o):int(o) + int(n)].tobytes() if n < 2**20 else int(n)
                  for o, n in zip(off, ol_)]


@pytest.mark.parametrize("suite,h,kl", SUITES, ids=["chacha20", "aes128", "aes256"])
def test_derived_keyring_equals_hkdf(ctx, suite, h, kl):
    rng = np.random.Generator(np.random.PCG64(900 + suite))
    secrets = [rng.bytes(h().digest_size) for _ in range(3)]
    sizes = [int(x) for x in rng.integers(2048, 2065, 16)] + [1, 15, 16, 63, 2500]
    kid = np.repeat(np.arange(6), len(sizes))
    pns = rng.integers(0, 2**40, len(kid))
    pkts = [packet(rng, sizes[i % len(sizes)], int(pn)) for i, pn in enumerate(pns)]
    with QuicKeyring.from_secrets(ctx, [QuicSecret.of(s) for s in secrets], suite) as kr:
        for newest in (1, 2, 3, 4):
            if newest > 1:
                kr.rekey([0, 1, 2])
            keys = [None] * 6
            for c in range(3):
                for g in (newest - 1, newest):
                    keys[2 * c + (g & 1)] = gen_key(h, kl, secrets[c], g)
            with QuicKeyring(ctx, keys, suite) as ref:
                # key_id NULL: entry 0 from the launch arguments (rewritten by
                # the first and third key update)
                for ids in (kid, None):
                    want = launch(ctx, sqobfs.quic_seal, ref, pkts, pns, ids)[2]
                    got = launch(ctx, sqobfs.quic_seal, kr, pkts, pns, ids)[2]
                    assert all(len(w) == len(p) + 16 for w, p in zip(want, pkts))
                    assert got == want, (newest, ids is None)


def test_rfc9001_a5_from_secret(ctx):
    a5 = json.load(open(ol.REPO + "/tests/golden/quic.json"))["rfc9001_a5"]
    pkt = B(a5["header"] + a5["payload"])
    with QuicKeyring.from_secrets(ctx, [QuicSecret.of(B(a5["secret"]))]) as kr:
        got = launch(ctx, sqobfs.quic_seal, kr, [pkt], [a5["pn"]], None, a5["pn_offset"])[2]
    assert got[0].hex() == a5["protected"]


@pytest.mark.parametrize("suite,h,kl", SUITES, ids=["chacha20", "aes128", "aes256"])
def test_key_phase(ctx, suite, h, kl):
    import torch

    rng = np.random.Generator(np.random.PCG64(950 + suite))
    secrets = [QuicSecret.of(rng.bytes(h().digest_size)) for _ in range(2)]
    sealed_with = [e for e in range(4) for _ in range(5)] + [2]
    pns = rng.integers(1, 2**30, len(sealed_with))
    pkts = [packet(rng, int(rng.integers(20, 300)), int(pn), e & 1)
            for e, pn in zip(sealed_with[:-1], pns)]
    pkts.append(packet(rng, 100, int(pns[-1]), 0, 0xC3))  # long header: no key phase
    with QuicKeyring.from_secrets(ctx, secrets, suite) as kr:
        prot = launch(ctx, sqobfs.quic_seal, kr, pkts, pns, sealed_with)[2]
        prot.append(rng.bytes(PNO + 19))  # too short to sample
        given = [e & ~1 for e in sealed_with] + [3]
        largest = np.concatenate([pns - 1, [0]])
        b, d, _ = launch(ctx, None, kr, prot, largest, given)
        ids = torch.from_numpy(np.full(len(prot), 0xFFFF, np.uint16)).to(d["in_"].device)
        wire = d["in_"].cpu().numpy().copy()
        sqobfs.quic_key_phase(ctx, kr, b, ids)
        ctx.sync()
        assert ids.cpu().numpy().tolist() == sealed_with + [3]
        assert np.array_equal(d["in_"].cpu().numpy(), wire), "the input is not modified"
        b, d, plain = launch(ctx, sqobfs.quic_open, kr, prot, largest, ids.cpu().numpy())
    assert plain == pkts + [sqobfs.QUIC_ESHORT]
    assert d["pn_out"].cpu().numpy().tolist() == pns.tolist() + [0]


def test_rekey_rejects(ctx):
    rng = np.random.Generator(np.random.PCG64(990))
    pkts, pns, kid = [packet(rng, 200, pn) for pn in range(4)], [0, 1, 2, 3], [0, 1, 2, 3]
    sec = [QuicSecret.of(rng.bytes(32)) for _ in range(2)]
    with QuicKeyring.from_secrets(ctx, sec) as kr, \
            QuicKeyring(ctx, [QuicKey.of(rng.bytes(32), rng.bytes(12), rng.bytes(32))]) as host:
        before = launch(ctx, sqobfs.quic_seal, kr, pkts, pns, kid)[2]
        for bad in ([0, 0], [2], [1, 0xFFFFFFFF]):
            for s in (None, sec[:len(bad)]):
                with pytest.raises(sqobfs.SqError):
                    kr.rekey(bad, s)
        with pytest.raises(sqobfs.SqError):
            host.rekey([0])  # made from keys: it has no secrets
        with pytest.raises(sqobfs.SqError):
            QuicKeyring.from_secrets(ctx, [sec[0]] * 32769)
        assert launch(ctx, sqobfs.quic_seal, kr, pkts, pns, kid)[2] == before
