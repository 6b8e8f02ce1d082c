"""QUIC Retry packets and their address-validation tokens on the GPU
(sqobfs_quic_retry / _retry_check and the _salamander forms), bit-exact
against the header's formats restated below over the CPU oracle's AES-GCM."""
from __future__ import annotations

import numpy as np
import pytest
import sqobfs
from sqobfs import (QUIC_EHEADER, QUIC_ESHORT, QUIC_TOKEN_BAD, QUIC_TOKEN_EHEADER,
                    QUIC_TOKEN_EXPIRED, QUIC_TOKEN_FOREIGN, QUIC_TOKEN_NONE, QUIC_TOKEN_OK, QuicKey)

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)
from test_gpu_quic_initial import initial
from test_gpu_quic_route import dev, place

pytestmark = pytest.mark.gpu
PSK = b"retry-test-psk"
RKEY, RNONCE = bytes.fromhex("be0c690b9f66575a1d766b54e368c84e"), bytes.fromhex("461599d35d632bf2239825bb")
TKEY, TIV = bytes(range(1, 17)), bytes(range(101, 113))
SLOT, FILL = 141, 0x5A  # output slots at odd offsets, sentinel-filled


def ref_retry(odcid, scid, rscid, token):
    body = b"\xf0\x00\x00\x00\x01" + bytes([len(scid)]) + scid + bytes([len(rscid)]) + rscid + token
    return body + ol.gcm_seal(RKEY, RNONCE, bytes([len(odcid)]) + odcid + body, b"")


def ref_token(nonce, addr, cid, now, odcid, key=TKEY):
    aad = addr + bytes([len(cid)]) + cid.ljust(20, b"\0")
    plain = now.to_bytes(4, "big") + bytes([len(odcid)]) + odcid.ljust(20, b"\0")
    return nonce + ol.gcm_seal(key, bytes(a ^ b for a, b in zip(TIV, nonce)), aad, plain)


def token_keyring(ctx, key=TKEY):
    return sqobfs.QuicKeyring(ctx, [QuicKey.of(key, TIV, bytes(16))], sqobfs.QUIC_AES_128_GCM)


def wrap(rng, pkts, salamander):
    return [ol.salamander_write(PSK, rng.bytes(8), p)[0] for p in pkts] if salamander else list(pkts)


def rows(rng, n, width):
    """n random width-byte rows: (list of bytes, device uint8 [n * width])."""
    a = rng.integers(0, 256, (n, width)).astype(np.uint8)
    return [r.tobytes() for r in a], dev(a.reshape(-1), np.uint8)


def retry(ctx, wires, okr, d_salt=None, **kw):
    """Retries of the datagrams: per datagram the output bytes or the error code."""
    n = len(wires)
    d_in, d_off, d_len, _, data = place(wires)
    out, out_len = dev(np.full(n * SLOT + 8, FILL), np.uint8), dev(np.full(n, 7), np.uint32)
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, out, dev(3 + SLOT * np.arange(n), np.uint64),
                          out_len, None, None)
    try:
        sqobfs.quic_retry(ctx, b, sqobfs.quic_retry_args(**kw), okr, d_salt)
    except sqobfs.SqError:
        ctx.sync()
        assert (out_len.cpu().numpy() == 7).all() and (out.cpu().numpy() == FILL).all(), \
            "refused, yet something was launched"
        raise
    ctx.sync()
    got, lens = out.cpu().numpy(), out_len.cpu().numpy()
    assert np.array_equal(d_in.cpu().numpy(), data), "the input is not modified"
    res = []
    for i, ln in enumerate(lens.tolist()):
        slot = got[3 + SLOT * i:3 + SLOT * (i + 1)]
        ln_ok = ln if ln < SLOT else 0
        assert (slot[ln_ok:] == FILL).all(), "written past the packet"
        res.append(slot[:ln].tobytes() if ln < SLOT else ln)
    return res


def check(ctx, wires, okr, **kw):
    n = len(wires)
    d_in, d_off, d_len, _, data = place(wires)
    st, od = dev(np.full(n, 99), np.uint8), dev(np.full(20 * n, 0xEE), np.uint8)
    odl, iat = dev(np.full(n, 0xEE), np.uint8), dev(np.full(n, 0xEEEEEEEE), np.uint32)
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, None, None, None, None, None)
    try:
        sqobfs.quic_retry_check(ctx, b, sqobfs.quic_retry_args(**kw), st, od, odl, iat, okr)
    except sqobfs.SqError:
        ctx.sync()
        assert (st.cpu().numpy() == 99).all(), "refused, yet something was launched"
        raise
    ctx.sync()
    st = st.cpu().numpy().tolist()
    assert np.array_equal(d_in.cpu().numpy(), data), "the input is not modified"
    od = od.cpu().numpy().reshape(n, 20)
    return st, [(od[i].tobytes(), v, t) for i, (v, t) in
                enumerate(zip(odl.cpu().numpy().tolist(), iat.cpu().numpy().tolist()))]


def test_retry_rfc9001_a4(ctx):
    odcid, rscid = bytes.fromhex("8394c8f03e515708"), bytes.fromhex("f067a5502a4262b5")
    pkt, _ = initial(odcid, b"", b"", 1, 2, 2, 2, bytes(40))
    got, = retry(ctx, [pkt], None, rscid=dev(np.frombuffer(rscid.ljust(20, b"\0"), np.uint8), np.uint8),
                 rscid_len=8, token=dev(np.frombuffer(b"token".ljust(64, b"\0"), np.uint8), np.uint8),
                 token_len=dev([5], np.uint8))
    rfc = bytes.fromhex("ff000000010008f067a5502a4262b5746f6b656e04a265ba2eff4d829058fb3f0f2496ba")
    # the vector's tag covers its first byte 0xff; ours is 0xf0 (the low nibble is unused)
    assert ol.gcm_seal(RKEY, RNONCE, b"\x08" + odcid + rfc[:-16], b"") == rfc[-16:]
    assert got[:1] == b"\xf0" and got[1:-16] == rfc[1:-16]
    assert got == ref_retry(odcid, b"", rscid, b"token")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("own", [False, True], ids=["library", "caller"])
@pytest.mark.parametrize("salamander", [False, True])
def test_retry_matches_reference(ctx, salamander, own, n):
    rng = np.random.Generator(np.random.PCG64(9100 + 8 * n + 2 * own + salamander))
    rl, now = [1, 8, 20][n % 3], 0x89ABCDEF
    pkts, want_plain = [], []
    addrs, d_addr = rows(rng, n, 18)
    nonces, d_nonce = rows(rng, n, 12)
    rscids, d_rscid = rows(rng, n, 20)
    tokens, d_token = rows(rng, n, 64)
    tls = [[1, 15, 16, 17, 64][(i // 12) % 5] for i in range(n)]
    salts, d_salt = rows(rng, n, 8)
    ends = set()
    for i in range(n):
        dcid, scid = rng.bytes([1, 8, 20][i % 3]), rng.bytes([0, 1, 8, 20][(i // 3) % 4])
        pkt, _ = initial(dcid, scid, rng.bytes(i % 5), 1, 2, i, 2, rng.bytes(30 + i % 7))
        bad = {5: bytes([0x40]) + pkt[1:],                 # short header
               6: bytes([0xE0]) + pkt[1:],                 # Handshake
               7: pkt[:1] + b"\x6b\x33\x43\xcf" + pkt[5:],  # v2
               8: pkt[:6 + len(dcid)]}.get(i % 11)         # cut before scid_len
        if bad is not None:
            pkts.append(bad)
            want_plain.append(QUIC_ESHORT if i % 11 == 8 else QUIC_EHEADER)
            continue
        tok = tokens[i][:tls[i]] if own else ref_token(nonces[i], addrs[i], rscids[i][:rl], now, dcid)
        pkts.append(pkt)
        want_plain.append(ref_retry(dcid, scid, rscids[i][:rl], tok))
        ends.add((1 + len(dcid) + len(want_plain[-1]) - 16) % 16)
    assert not (own and n == 257) or {15, 0, 1} <= ends, "pseudo-packet lengths around a block's end"
    want = [ol.salamander_write(PSK, s, w)[0] if salamander and isinstance(w, bytes) else w
            for s, w in zip(salts, want_plain)]
    kw = dict(token=d_token, token_len=dev(tls, np.uint8)) if own else \
        dict(addr=d_addr, nonce=d_nonce, now=now)
    with token_keyring(ctx) as tkr, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        got = retry(ctx, wrap(rng, pkts, salamander), okr if salamander else None, d_salt,
                    rscid=d_rscid, rscid_len=rl, **(kw if own else dict(kw, tkr=tkr)))
    assert got == want


KINDS = ["ok", "nonce", "cipher", "tag", "addr", "dcid", "none", "short52", "handshake"]


@pytest.mark.parametrize("tok_vl", [1, 2])
@pytest.mark.parametrize("cids", ["short", "long"])
@pytest.mark.parametrize("salamander", [False, True])
def test_retry_round_trip_and_check(ctx, salamander, cids, tok_vl):
    """short: the token starts before packet byte 32 and ends after it; long
    (20-byte ids): it lies wholly past byte 32."""
    rng = np.random.Generator(np.random.PCG64(9200 + 4 * salamander + 2 * (cids == "long") + tok_vl))
    n, rl, now, max_age = 70, *((1, 5000, 10) if cids == "short" else (20, 0xFFFFFFF0, 100))
    addrs, d_addr = rows(rng, n, 18)
    _, d_nonce = rows(rng, n, 12)
    rscids, d_rscid = rows(rng, n, 20)
    _, d_salt = rows(rng, n, 8)
    dcids = [rng.bytes([1, 8, 20][i % 3]) for i in range(n)]
    scids = [rng.bytes(0 if cids == "short" else 20) for i in range(n)]
    first = [initial(d, s, b"", 1, 2, 0, 2, rng.bytes(40))[0] for d, s in zip(dcids, scids)]
    flip = lambda t, k: t[:k] + bytes([t[k] ^ (1 << k % 8)]) + t[k + 1:]  # noqa: E731
    with token_keyring(ctx) as tkr, token_keyring(ctx, bytes(16)) as other, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr0:
        okr = okr0 if salamander else None
        got = retry(ctx, wrap(rng, first, salamander), okr, d_salt, tkr=tkr, addr=d_addr,
                    nonce=d_nonce, rscid=d_rscid, rscid_len=rl, now=now)
        second, addr2 = [], [bytearray(a) for a in addrs]
        for i, r in enumerate(got):
            if salamander:
                key = ol.salamander_key(PSK, r[:8])
                r = bytes(c ^ key[k % 32] for k, c in enumerate(r[8:]))
            tok, kind = r[7 + len(scids[i]) + rl:-16], KINDS[i % len(KINDS)]
            start = 7 + rl + len(scids[i]) + tok_vl  # of the token in the next Initial
            assert len(tok) == 53 and (start < 32 < start + 53 if cids == "short" else start > 32)
            dcid = rscids[i][:rl]
            tok = {"nonce": flip(tok, i % 12), "cipher": flip(tok, 12 + i % 25),
                   "tag": flip(tok, 37 + i % 16), "none": b"", "short52": tok[:52]}.get(kind, tok)
            if kind == "addr":
                addr2[i][i % 18] ^= 0x10
            if kind == "dcid":
                dcid = flip(dcid, i % rl)
            second.append(initial(dcid, scids[i], tok, 1 if not tok else tok_vl, 2, 1, 2, rng.bytes(40),
                                  first=0xE0 if kind == "handshake" else 0xC0)[0])
        wires = wrap(rng, second, salamander)
        d_addr2 = dev(np.frombuffer(b"".join(map(bytes, addr2)), np.uint8), np.uint8)
        fixed = {"none": QUIC_TOKEN_NONE, "short52": QUIC_TOKEN_FOREIGN, "handshake": QUIC_TOKEN_EHEADER}
        for key, t, valid in [(tkr, now + max_age, QUIC_TOKEN_OK), (other, now, QUIC_TOKEN_BAD),
                              (tkr, now + max_age + 1, QUIC_TOKEN_EXPIRED),
                              (tkr, now - 1, QUIC_TOKEN_EXPIRED)]:
            st, outs = check(ctx, wires, okr, tkr=key, addr=d_addr2, now=t & 0xFFFFFFFF, max_age=max_age)
            for i in range(n):
                kind = KINDS[i % len(KINDS)]
                assert st[i] == fixed.get(kind, valid if kind == "ok" else QUIC_TOKEN_BAD), (i, kind)
                written = st[i] in (QUIC_TOKEN_OK, QUIC_TOKEN_EXPIRED)
                assert outs[i] == ((dcids[i].ljust(20, b"\0"), len(dcids[i]), now) if written else
                                   (b"\xEE" * 20, 0xEE, 0xEEEEEEEE)), (i, kind)


def test_retry_refusals(ctx):
    rng = np.random.Generator(np.random.PCG64(9300))
    pkts = [initial(rng.bytes(8), rng.bytes(4), b"", 1, 2, 0, 2, rng.bytes(40))[0] for _ in range(3)]
    _, d18 = rows(rng, 3, 18)
    _, d64 = rows(rng, 3, 64)
    with token_keyring(ctx) as tkr, sqobfs.Context(0) as ctx2, token_keyring(ctx2) as tkr2, \
            sqobfs.QuicKeyring(ctx, [QuicKey.of(bytes(32), TIV, bytes(32))]) as chacha, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr, \
            sqobfs.Keyring(ctx, sqobfs.XPLUS, [PSK]) as xkr, \
            sqobfs.Keyring(ctx2, sqobfs.SALAMANDER, [PSK]) as okr2:
        good = dict(tkr=tkr, addr=d18, nonce=d64, rscid=d64, rscid_len=8)
        assert all(isinstance(r, bytes) for r in retry(ctx, pkts, None, **good))
        assert all(isinstance(r, bytes) for r in retry(ctx, wrap(rng, pkts, True), okr, d64, **good))
        cases = [(None, d64, dict(good, **{k: None})) for k in ("tkr", "addr", "nonce", "rscid")] + \
            [(None, d64, dict(good, tkr=k)) for k in (chacha, tkr2)] + \
            [(None, d64, dict(good, token=d64)), (None, d64, dict(good, token_len=d64))] + \
            [(None, d64, dict(good, rscid_len=k)) for k in (0, 21)] + \
            [(xkr, d64, good), (okr2, d64, good), (okr, None, good)]
        for kr, salt, kw in cases:
            with pytest.raises(sqobfs.SqError) as e:  # (retry: out_len keeps its fill, = 7 >= SLOT fails)
                retry(ctx, wrap(rng, pkts, kr is not None), kr, salt, **kw)
            assert e.value.status == sqobfs.SQ_EINVAL, kw
        for kr, kw in [(None, dict(tkr=None)), (None, dict(addr=None)), (None, dict(tkr=chacha)),
                       (None, dict(tkr=tkr2)), (xkr, {}), (okr2, {})]:
            with pytest.raises(sqobfs.SqError) as e:
                check(ctx, pkts, kr, **dict(dict(tkr=tkr, addr=d18), **kw))
            assert e.value.status == sqobfs.SQ_EINVAL, kw
        d_in, d_off, d_len, _, _ = place(pkts)
        for bad in ("pn_offset", "pn", "key_id", "pn_out"):
            b = sqobfs.quic_batch(3, d_in, d_off, d_len, d64, d_off, dev([7] * 3, np.uint32),
                                  **{"pn_offset": None, "pn": None, bad: d64})
            with pytest.raises(sqobfs.SqError) as e:
                sqobfs.quic_retry(ctx, b, sqobfs.quic_retry_args(**good))
            assert e.value.status == sqobfs.SQ_EINVAL, bad
