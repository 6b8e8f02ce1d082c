"""QUIC stateless resets on the GPU (sqobfs_quic_reset / _reset_match, the
_salamander forms and the map's token table), bit-exact against Python's hmac
and the CPU oracle's ChaCha20 and Salamander."""
from __future__ import annotations

import hashlib
import hmac

import numpy as np
import pytest
import sqobfs
from sqobfs import QUIC_CID_REMOVE, QUIC_EHEADER, QUIC_ESHORT, QUIC_NOCONN

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)
from test_gpu_quic_route import dev, place

pytestmark = pytest.mark.gpu
PSK = b"reset-test-psk"
KEY, SKEY = bytes(range(50, 82)), bytes(range(200, 232))  # reset key; the context's salt key
SLOT, FILL = 91, 0x5A  # output slots at odd offsets, sentinel-filled
NS = [1, 63, 64, 65, 257]  # 257: one more than the workgroup


def token(cid, key=KEY):
    return hmac.new(key, cid, hashlib.sha256).digest()[:16]


def short(rng, length, cid=b"", tail=b""):
    """A short-header packet of `length` bytes: first byte, cid, random, tail."""
    body = cid + rng.bytes(length - 1 - len(cid) - len(tail)) + tail
    return bytes([0x40 | rng.integers(0, 64)]) + body


def wrap(rng, pkts, salamander):
    return [ol.salamander_write(PSK, rng.bytes(8), p)[0] for p in pkts] if salamander else list(pkts)


def reset(ctx, wires, okr, d_salt, cid_len, reset_len, key=KEY, out=True, **bad):
    """Resets of the datagrams: per datagram the output bytes or the error code."""
    n = len(wires)
    d_in, d_off, d_len, _, data = place(wires)
    buf, out_len = dev(np.full(n * SLOT + 8, FILL), np.uint8), dev(np.full(n, 7), np.uint32)
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, buf if out else None,
                          dev(3 + SLOT * np.arange(n), np.uint64), out_len, None, None)
    for k, v in bad.items():
        setattr(b, k, v)
    try:
        sqobfs.quic_reset(ctx, b, key, cid_len, reset_len, okr, d_salt)
    except sqobfs.SqError:
        ctx.sync()
        assert (out_len.cpu().numpy() == 7).all() and (buf.cpu().numpy() == FILL).all(), \
            "refused, yet something was launched"
        raise
    ctx.sync()
    got, lens = buf.cpu().numpy(), out_len.cpu().numpy()
    assert np.array_equal(d_in.cpu().numpy(), data), "the input is not modified"
    assert (got[:3] == FILL).all()
    res = []
    for i, ln in enumerate(lens.tolist()):
        slot = got[3 + SLOT * i:3 + SLOT * (i + 1)]
        assert (slot[ln if ln < SLOT else 0:] == FILL).all(), "written past the packet"
        res.append(slot[:ln].tobytes() if ln < SLOT else ln)
    return res


def match(ctx, cmap, wires, okr, conn_out=True, **bad):
    """(conn_out as a list, hits) of the datagrams."""
    n = len(wires)
    d_in, d_off, d_len, _, data = place(wires)
    conn, hits = dev(np.full(n, 12345), np.uint32), dev([0], np.uint32)
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, None, None, None, None, None)
    for k, v in bad.items():
        setattr(b, k, v)
    try:
        sqobfs.quic_reset_match(ctx, cmap, b, conn if conn_out else None, hits, okr)
    except sqobfs.SqError:
        ctx.sync()
        assert (conn.cpu().numpy() == 12345).all() and int(hits.cpu()[0]) == 0, \
            "refused, yet something was launched"
        raise
    ctx.sync()
    assert np.array_equal(d_in.cpu().numpy(), data), "the input is not modified"
    return conn.cpu().numpy().tolist(), int(hits.cpu()[0])


def ref_reset(pkt, i, seq, cid_len, reset_len):
    if len(pkt) < 22:
        return QUIC_ESHORT
    r = min(reset_len, len(pkt) - 1)
    fill = ol.chacha20_stream(SKEY, b"sqsr" + seq.to_bytes(8, "little"), i, r - 16)
    return bytes([(fill[0] & 0x3F) | 0x40]) + fill[1:] + token(pkt[1:1 + cid_len])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cid_len,reset_len", [(1, 21), (8, 42), (20, 80)])
@pytest.mark.parametrize("salamander", [False, True])
def test_reset_matches_reference(ctx, salamander, cid_len, reset_len, n):
    rng = np.random.Generator(np.random.PCG64(9400 + 1000 * salamander + 10 * reset_len + n))
    cycle = [21, 22, 23, reset_len, reset_len + 1, reset_len + 2, 1350]
    pkts = [short(rng, cycle[i % 7]) for i in range(n)]
    salts = rng.integers(0, 256, (n, 8)).astype(np.uint8)
    d_salt, seq = dev(salts.reshape(-1), np.uint8), 0x1_0000_0005
    ctx.salt_key(SKEY, seq)
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr0:
        okr, wires, prev = okr0 if salamander else None, wrap(rng, pkts, salamander), None
        for call in range(2):  # the second: other filler, the same tokens
            got = reset(ctx, wires, okr, d_salt, cid_len, reset_len)
            assert ctx.salt_seq == seq + call + 1
            want = [ref_reset(p, i, seq + call, cid_len, reset_len) for i, p in enumerate(pkts)]
            if salamander:
                want = [ol.salamander_write(PSK, s.tobytes(), w)[0] if isinstance(w, bytes) else w
                        for s, w in zip(salts, want)]
            assert got == want
            for g, p in zip(got, prev or []):
                assert not isinstance(g, bytes) or (g[-16:] == p[-16:] and g[:-16] != p[:-16])
            prev = got


@pytest.mark.parametrize("salamander", [False, True])
def test_reset_header_rejects(ctx, salamander):
    rng = np.random.Generator(np.random.PCG64(9500 + salamander))
    good = short(rng, 60)
    pkts = [bytes([0xC3]) + good[1:], bytes([0x80]) + good[1:9], bytes([0x3F]) + good[1:], good]
    wires = wrap(rng, pkts, salamander) + ([rng.bytes(8), rng.bytes(3)] if salamander else [b""])
    ctx.salt_key(SKEY, 77)
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        got = reset(ctx, wires, okr if salamander else None, dev(np.zeros(48), np.uint8), 8, 40)
    assert got[:3] == [QUIC_EHEADER] * 3 and got[4:] == [QUIC_ESHORT] * (len(wires) - 4)
    want = ref_reset(good, 3, 77, 8, 40)
    assert got[3] == (ol.salamander_write(PSK, bytes(8), want)[0] if salamander else want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("salamander", [False, True])
def test_match(ctx, salamander, n):
    rng = np.random.Generator(np.random.PCG64(9600 + 1000 * salamander + n))
    conns, m = 16, 40
    toks = [rng.bytes(16) for _ in range(m)]
    conn_of = {t: j % conns for j, t in enumerate(toks)}
    pkts, want = [], []
    for i in range(n):
        t, kind, length = toks[i % m], i % 9, 21 + i % 32
        if kind == 1:  # one bit of word (i // 9) % 4
            k = 4 * ((i // 9) % 4) + i % 4
            t = t[:k] + bytes([t[k] ^ (1 << i % 8)]) + t[k + 1:]
        p = short(rng, 20 if kind == 3 else length, tail=t)  # 3: too short for a reset
        if kind == 2:  # a long header
            p = bytes([p[0] | 0x80]) + p[1:]
        pkts.append(p)
        # token 3 is removed below and token 5 re-mapped to connection 7
        want.append(QUIC_NOCONN if kind in (1, 2, 3) or i % m == 3 else 7 if i % m == 5 else
                    conn_of[t])
    with sqobfs.QuicCidMap(ctx, conns, m, 8) as cmap, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        cmap.update_reset([(t, c) for t, c in conn_of.items()])  # max_cids tokens: full load
        cmap.update_reset([(toks[3], QUIC_CID_REMOVE), (rng.bytes(16), QUIC_CID_REMOVE), (toks[5], 7)])
        got, hits = match(ctx, cmap, wrap(rng, pkts, salamander), okr if salamander else None)
    assert got == want and hits == sum(w != QUIC_NOCONN for w in want)


@pytest.mark.parametrize("salamander", [False, True])
def test_match_without_tokens(ctx, salamander):
    rng = np.random.Generator(np.random.PCG64(9700 + salamander))
    wires = wrap(rng, [short(rng, 21 + i % 32) for i in range(65)], salamander)
    with sqobfs.QuicCidMap(ctx, 4, 4, 8) as cmap, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        assert match(ctx, cmap, wires, okr if salamander else None) == ([QUIC_NOCONN] * 65, 0)


def test_reset_round_trip_salamander(ctx):
    rng = np.random.Generator(np.random.PCG64(9800))
    n = 70
    cids = [rng.bytes(8) for _ in range(n)]
    wires = wrap(rng, [short(rng, 30 + i, cid=c) for i, c in enumerate(cids)], True)
    d_salt = dev(rng.integers(0, 256, 8 * n), np.uint8)
    with sqobfs.QuicCidMap(ctx, n, n, 8) as cmap, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        resets = reset(ctx, wires, okr, d_salt, 8, 50)
        for i, (r, c) in enumerate(zip(resets, cids)):
            plain, ln = ol.salamander_read(PSK, r)
            assert ln == min(50, 29 + i) and plain[:ln][-16:] == token(c), i
        cmap.update_reset([(token(c), i) for i, c in enumerate(cids)])
        assert match(ctx, cmap, resets, okr) == (list(range(n)), n)


def test_reset_refusals(ctx):
    rng = np.random.Generator(np.random.PCG64(9900))
    pkts = [short(rng, 40) for _ in range(3)]
    d64 = dev(rng.integers(0, 256, 64), np.uint8)
    toks = [rng.bytes(16) for _ in range(6)]
    ends = [short(rng, 30, tail=t) for t in toks]
    with sqobfs.Context(0) as ctx2, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr, \
            sqobfs.Keyring(ctx, sqobfs.XPLUS, [PSK]) as xkr, \
            sqobfs.Keyring(ctx2, sqobfs.SALAMANDER, [PSK]) as okr2, \
            sqobfs.QuicCidMap(ctx, 4, 4, 8) as cmap, sqobfs.QuicCidMap(ctx2, 4, 4, 8) as cmap2:
        assert all(isinstance(r, bytes) for r in reset(ctx, pkts, None, None, 8, 30))
        assert all(isinstance(r, bytes) for r in reset(ctx, wrap(rng, pkts, True), okr, d64, 8, 30))
        ptr = d64.data_ptr()
        cases = [(None, None, dict(cid_len=c, reset_len=30)) for c in (0, 21)] + \
            [(None, None, dict(cid_len=8, reset_len=r)) for r in (20, 81)] + \
            [(None, None, dict(cid_len=8, reset_len=30, **{f: v})) for f, v in
             [("pn_offset", ptr), ("pn", ptr), ("key_id", ptr), ("pn_out", ptr), ("flags", 1),
              ("in_len", None), ("out_off", None), ("out_len", None), ("out", False)]] + \
            [(kr, salt, dict(cid_len=8, reset_len=30)) for kr, salt in
             [(xkr, d64), (okr2, d64), (okr, None)]]
        for kr, salt, kw in cases:
            with pytest.raises(sqobfs.SqError) as e:
                reset(ctx, wrap(rng, pkts, kr is not None), kr, salt, **kw)
            assert e.value.status == sqobfs.SQ_EINVAL, kw
        cmap.update_reset([(t, j) for j, t in enumerate(toks[:4])])
        for ops in ([(toks[4], 0)], [(toks[0], QUIC_CID_REMOVE), (toks[4], 1), (toks[5], 2)],
                    [(toks[0], 4)]):  # past max_cids (twice), conn >= conns
            with pytest.raises(sqobfs.SqError) as e:
                cmap.update_reset(ops)
            assert e.value.status == sqobfs.SQ_EINVAL, ops
        assert match(ctx, cmap, ends, None) == ([0, 1, 2, 3, QUIC_NOCONN, QUIC_NOCONN], 4)
        for m, kr, kw in [(cmap2, None, {}), (cmap, xkr, {}), (cmap, okr2, {}),
                          (cmap, None, dict(conn_out=False)), (cmap, None, dict(out=ptr)),
                          (cmap, None, dict(out_len=ptr)), (cmap, None, dict(pn=ptr)),
                          (cmap, None, dict(flags=1)), (cmap, None, dict(in_off=None))]:
            with pytest.raises(sqobfs.SqError) as e:
                match(ctx, m, ends, kr, **kw)
            assert e.value.status == sqobfs.SQ_EINVAL, kw
