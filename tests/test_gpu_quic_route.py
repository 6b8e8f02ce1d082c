"""Routing received QUIC datagrams on the GPU (sqobfs_quic_cidmap_*,
sqobfs_quic_route / _route_salamander).  The routing reference is a Python
dict and ref_class below, which restates the header's class table; packets
for the chained test are sealed by the CPU oracle with HKDF keys from hmac /
hashlib, as the key-update and Initial tests do."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import sqobfs
from sqobfs import (QUIC_CID_REMOVE, QUIC_EAUTH, QUIC_NOCONN, QUIC_ROUTE_HANDSHAKE,
                    QUIC_ROUTE_INITIAL, QUIC_ROUTE_MALFORMED, QUIC_ROUTE_OTHER, QUIC_ROUTE_SHORT,
                    QUIC_ROUTE_UNKNOWN, QUIC_ROUTE_ZERO_RTT, QUIC_SIDE_CLIENT, QuicSecret)

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)
from test_gpu_quic_initial import initial, initial_keys, varint
from test_gpu_quic_keys import gen_key

pytestmark = pytest.mark.gpu
PSK = b"route-test-psk"
BAD = (QUIC_ROUTE_MALFORMED, QUIC_NOCONN, 0, None)


def ref_class(p, cl, table):
    """(class, conn, pn_offset, span or None) of packet p for a map of cl-byte ids."""
    if not p:
        return BAD
    if not p[0] & 0x80:
        if not p[0] & 0x40 or len(p) < 1 + cl:
            return BAD
        c = table.get(p[1:1 + cl])
        return (QUIC_ROUTE_UNKNOWN, QUIC_NOCONN, 0, None) if c is None else \
            (QUIC_ROUTE_SHORT, c, 1 + cl, None)
    if len(p) < 5:
        return BAD
    if int.from_bytes(p[1:5], "big") != 1 or (p[0] & 0x70) == 0x70:
        return QUIC_ROUTE_OTHER, QUIC_NOCONN, 0, None
    if not p[0] & 0x40 or len(p) < 6 or p[5] > 20 or 6 + p[5] > len(p):
        return BAD
    dl, t = p[5], (p[0] >> 4) & 3
    dcid = p[6:6 + dl]
    if t == 0:
        return QUIC_ROUTE_INITIAL, table.get(dcid, QUIC_NOCONN) if dl == cl else QUIC_NOCONN, 0, None
    if 6 + dl >= len(p) or p[6 + dl] > 20 or 7 + dl + p[6 + dl] >= len(p):
        return BAD
    q = 7 + dl + p[6 + dl]
    nb = 1 << (p[q] >> 6)
    if q + nb > len(p):
        return BAD
    length = int.from_bytes(p[q:q + nb], "big") & ((1 << (8 * nb - 2)) - 1)
    if q + nb + length > len(p):
        return BAD
    if dl != cl or dcid not in table:
        return QUIC_ROUTE_UNKNOWN, QUIC_NOCONN, 0, None
    return QUIC_ROUTE_HANDSHAKE if t == 2 else QUIC_ROUTE_ZERO_RTT, table[dcid], q + nb, q + nb + length


def dev(a, dt):
    import torch
    return torch.from_numpy(np.array(a, dt)).to(torch.device("cuda", 0))


def place(wires):
    """The datagrams at ragged offsets: device buffer, in_off, in_len (numpy offsets too)."""
    lens = np.array([len(w) for w in wires], np.uint32)
    off = np.concatenate([[5], 5 + np.cumsum(lens + 3)]).astype(np.uint64)
    data = np.full(int(off[-1]) + 16, 0xA5, np.uint8)
    for o, w in zip(off, wires):
        data[int(o):int(o) + len(w)] = np.frombuffer(w, np.uint8)
    return dev(data, np.uint8), dev(off[:-1], np.uint64), dev(lens, np.uint32), off[:-1], data


def route(ctx, cmap, okr, d_in, d_off, d_len, d_out_off=None, **bad):
    import torch
    n = d_len.numel()
    r = sqobfs.QuicRouted(n, d_in.device, d_out_off is not None)
    r.count = dev(np.full(8, 7), np.uint32)
    extra = {k: dev(np.zeros(n), np.uint64 if k == "pn" else np.uint16) for k in bad}
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, None, d_out_off, None, extra.get("pn_offset"),
                          extra.get("pn"), extra.get("key_id"))
    torch.cuda.synchronize()
    try:
        if okr is None:
            sqobfs.quic_route(ctx, cmap, b, r)
        else:
            sqobfs.quic_route_salamander(ctx, cmap, okr, b, r)
    except sqobfs.SqError:
        ctx.sync()
        assert r.count.cpu().numpy().tolist() == [7] * 8, "refused, yet something was launched"
        raise
    ctx.sync()
    return r


def near(rng, cid, table):
    """An id that differs from the registered cid in its last byte only."""
    while True:
        c = cid[:-1] + bytes([cid[-1] ^ int(rng.integers(1, 256))])
        if c not in table:
            return c


def long_hdr(first, dcid, scid, rest=b"", version=1, dlen=None, slen=None):
    return bytes([first]) + version.to_bytes(4, "big") + \
        bytes([len(dcid) if dlen is None else dlen]) + dcid + \
        bytes([len(scid) if slen is None else slen]) + scid + rest


def datagrams(rng, cl, table, salamander, skip_zero_rtt):
    """700 packets in random order over every class and cause of the table."""
    live = sorted(table)
    pick = lambda: live[int(rng.integers(len(live)))]  # noqa: E731
    body = lambda: rng.bytes(int(rng.integers(0, 60)))  # noqa: E731
    hs = lambda first, dcid, i, cut=0, extra=0: long_hdr(  # noqa: E731
        first | (i & 15), dcid, rng.bytes([0, 20][i % 2]),
        varint(40 + extra, [1, 2, 4, 8][(i // 2) % 4]) + rng.bytes(40 - cut + (i % 3) * 7 * (not cut)))
    odd = cl + 1 if cl < 20 else cl - 1
    makers = [
        lambda i: bytes([0x40 | (i & 0x3F)]) + pick() + body(),
        lambda i: bytes([0x7F]) + pick(),                               # exactly 1 + cid_len
        lambda i: bytes([0x40]) + near(rng, pick(), table) + body(),    # unknown id
        lambda i: bytes([0x3F & i]) + pick() + body(),                  # fixed bit clear
        lambda i: bytes([0x41]) + pick()[:cl - 1],                      # shorter than the id
        lambda i: b"",
        lambda i: long_hdr(0xC0 | (i & 15), pick(), rng.bytes(5), body()),
        lambda i: long_hdr(0xC3, rng.bytes([0, 8, 20][i % 3] + (cl in (8, 20))), b"", body()),
        lambda i: long_hdr(0xC1, near(rng, pick(), table), rng.bytes(20), body()),
        lambda i: long_hdr(0xC0, b"", b"")[:6],                         # ends with dcid_len 0
        lambda i: hs(0xE0, pick(), i),                                  # Handshake (+ coalesced)
        lambda i: hs(0xE0 if skip_zero_rtt else 0xD0, pick(), i),       # 0-RTT
        lambda i: hs(0xE0, near(rng, pick(), table), i),                # unknown id
        lambda i: hs(0xD0, rng.bytes(odd), i),                          # dcid_len != cid_len
        lambda i: long_hdr(0x80 | (i & 0x7F), rng.bytes(8), b"", body(), version=0),
        lambda i: long_hdr(0xE0, pick(), b"", body(), version=0x6B3343CF),
        lambda i: long_hdr(0xF0 | (i & 15), pick(), rng.bytes(4), body()),  # Retry
        lambda i: b"\xC0\x00\x00\x00"[:1 + i % 4],                      # no room for a version
        lambda i: long_hdr(0x80 | (i & 0x30), pick(), b"", body()),     # v1, fixed bit clear
        lambda i: long_hdr(0xC0, rng.bytes(21), b"", body(), dlen=21),
        lambda i: long_hdr(0xC0, rng.bytes(8), b"")[:9],                # cut inside the DCID
        lambda i: long_hdr(0xE0, pick(), b"")[:6 + cl],                 # no scid_len
        lambda i: long_hdr(0xD0, pick(), rng.bytes(21), body(), slen=21),
        lambda i: hs(0xE0, pick(), i)[:7 + cl + 20 * (i % 2) + (i // 2) % 4],  # inside the varint
        lambda i: hs(0xE0, pick(), i, cut=1 + i % 5),                   # span past the end
    ]
    pkts = [makers[i % len(makers)](i) for i in range(700 - 9 * salamander)]
    wires = [ol.salamander_write(PSK, rng.bytes(8), p)[0] for p in pkts] if salamander else list(pkts)
    if salamander:  # wire datagrams too short for a salt and a byte
        wires += [rng.bytes(k) for k in range(9)]
        pkts += [b""] * 9
    perm = rng.permutation(len(pkts))
    return [pkts[i] for i in perm], [wires[i] for i in perm]


@pytest.mark.parametrize("salamander", [False, True])
@pytest.mark.parametrize("cl", [1, 4, 8, 20])
def test_route_matches_reference(ctx, cl, salamander):
    rng = np.random.Generator(np.random.PCG64(8100 + 2 * cl + salamander))
    conns, table = 40, {}
    with sqobfs.QuicCidMap(ctx, conns, 64, cl) as cmap, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr:
        # 64 ids in 128 slots over 40 connections; every third removed again (from
        # inside probe chains), half of those back under another connection, new
        # ones up to 64: the table is half full when the batch is routed
        cids = []
        while len(cids) < 64 + 11:
            c = rng.bytes(cl)
            if c not in cids:
                cids.append(c)
        steps = [[(c, i % conns) for i, c in enumerate(cids[:64])],
                 [(c, QUIC_CID_REMOVE) for c in cids[:63:3]] + [(cids[70], QUIC_CID_REMOVE)],
                 [(c, 39 - i) for i, c in enumerate(cids[:30:3])] + [(cids[1], 7)] +
                 [(c, 3) for c in cids[64:]]]
        for ops in steps:
            cmap.update(ops)
            for c, conn in ops:
                table.pop(c, None) if conn == QUIC_CID_REMOVE else table.update({c: conn})
        assert len(table) == 64 and len(set(table.values())) < 64
        # pn_state through commit: several packets per connection, failed ones, NOCONN
        pn_ref = np.zeros((conns, 3), np.uint64)
        for space in range(3):
            cj = rng.integers(0, conns + 3, 150).astype(np.uint32)
            cj[cj >= conns] = QUIC_NOCONN
            pj = rng.integers(1, 2**40, 150).astype(np.uint64)
            lj = rng.choice(np.array([100, 0, QUIC_EAUTH, 0xFFFFFFFC, 0xFFFFFFFF], np.uint32), 150)
            cmap.commit(space, 150, dev(cj, np.uint32), dev(lj, np.uint32), dev(pj, np.uint64))
            for c, ln, pn in zip(cj, lj, pj):
                if c != QUIC_NOCONN and ln < 0xFFFFFFFC:
                    pn_ref[c, space] = max(pn_ref[c, space], pn)
        pkts, wires = datagrams(rng, cl, table, salamander, cl == 1 and not salamander)
        d_in, d_off, d_len, off, data = place(wires)
        r = route(ctx, cmap, okr if salamander else None, d_in, d_off, d_len, dev(off + 77, np.uint64))
        assert np.array_equal(d_in.cpu().numpy(), data), "the input is not modified"
    want = []
    for p, w in zip(pkts, wires):
        cls, conn, pno, span = ref_class(p, cl, table)
        space = {QUIC_ROUTE_INITIAL: 0, QUIC_ROUTE_HANDSHAKE: 1}.get(cls, 2)
        keyed = cls in (QUIC_ROUTE_SHORT, QUIC_ROUTE_HANDSHAKE, QUIC_ROUTE_ZERO_RTT)
        want.append((cls, conn, pno, len(w) if span is None else span + 8 * salamander,
                     int(pn_ref[conn, space]) if conn != QUIC_NOCONN else 0, 2 * conn * keyed))
    cls = np.array([x[0] for x in want])
    counts = np.bincount(cls, minlength=8)
    assert (counts > 0).tolist() == [True] * 3 + [not (cl == 1 and not salamander)] + [True] * 3 + [False]
    order = np.argsort(cls, kind="stable")
    got = {k: getattr(r, k).cpu().numpy() for k, _ in r.FIELDS}
    assert got["cls"].tolist() == cls.tolist() and got["count"].tolist() == counts.tolist()
    assert got["order"].tolist() == order.tolist()
    assert got["in_off"].tolist() == off[order].tolist()
    assert got["out_off"].tolist() == (off[order] + 77).tolist()
    for k, col in (("conn", 1), ("pn_offset", 2), ("in_len", 3), ("pn", 4), ("key_id", 5)):
        assert got[k].tolist() == [want[i][col] for i in order], k


def short_packets(rng, suite, secrets, cids, pns, pn_len):
    """Per packet number one short-header packet of connection i % 2, key phase
    (i // 2) % 2: (unprotected, protected by the oracle with that generation's keys)."""
    h, kl, osuite = hashlib.sha256, *((32, ol.CHACHA20) if suite == sqobfs.QUIC_CHACHA20_POLY1305
                                      else (16, ol.AES128GCM))
    out = []
    for i, pn in enumerate(pns):
        c, g = i % 2, (i // 2) % 2
        k = gen_key(h, kl, secrets[c], g)
        pkt = bytes([0x40 | (g << 2) | (pn_len - 1)]) + cids[c] + \
            (pn % 256**pn_len).to_bytes(pn_len, "big") + rng.bytes(int(rng.integers(20, 300)))
        prot, rc = ol.quic_seal(bytes(k.key)[:kl], bytes(k.iv), bytes(k.hp)[:kl], pn, pkt, 9, osuite)
        assert rc == len(pkt) + 16
        out.append((pkt, prot))
    return out


def route_and_open(ctx, cmap, kr, okr, wires, commit):
    """route -> key_phase -> open on the SHORT slice (and initial_open on the
    INITIAL slice), the host reading only count; returns per class the input
    indices, outputs, out_len and pn_out."""
    d_in, d_off, d_len, off, _ = place(wires)
    d_out = dev(np.zeros(d_in.numel()), np.uint8)
    r = route(ctx, cmap, okr, d_in, d_off, d_len, d_off)
    counts, res = r.counts(), {}
    for cls in (QUIC_ROUTE_SHORT, QUIC_ROUTE_INITIAL):
        m = counts[cls]
        out_len, pn_out = dev(np.zeros(max(m, 1)), np.uint32), dev(np.zeros(max(m, 1)), np.uint64)
        b = r.batch(cls, counts, d_in, d_out, out_len, pn_out)
        if cls == QUIC_ROUTE_SHORT:
            ids = dev(np.zeros(max(m, 1)), np.uint16)
            if okr is None:
                sqobfs.quic_key_phase(ctx, kr, b, ids)
            else:
                sqobfs.quic_key_phase_salamander(ctx, kr, okr, b, ids)
            b.key_id = ids.data_ptr()
            sqobfs.quic_open(ctx, kr, b) if okr is None else sqobfs.quic_open_salamander(ctx, kr, okr, b)
            if commit:
                cmap.commit(2, m, r.conn[:m], out_len, pn_out)
        elif okr is None:
            sqobfs.quic_initial_open(ctx, b, QUIC_SIDE_CLIENT)
        else:
            sqobfs.quic_initial_open_salamander(ctx, okr, b, QUIC_SIDE_CLIENT)
        res[cls] = (out_len, pn_out)
    ctx.sync()
    buf, order, lo = d_out.cpu().numpy(), r.order.cpu().numpy(), 0
    for cls in sorted(res):
        ln, pn = (t.cpu().numpy()[:counts[cls]] for t in res[cls])
        idx = order[lo:lo + counts[cls]].tolist()
        res[cls] = (idx, [buf[int(off[i]):int(off[i]) + int(m)].tobytes() if m < 2**20 else int(m)
                          for i, m in zip(idx, ln)], pn.tolist())
        lo += counts[cls]
    return counts, res


@pytest.mark.parametrize("salamander", [False, True])
@pytest.mark.parametrize("suite", [sqobfs.QUIC_AES_128_GCM, sqobfs.QUIC_CHACHA20_POLY1305],
                         ids=["aes128", "chacha20"])
def test_route_feeds_open_and_commit(ctx, suite, salamander):
    """Batch B's 1-byte packet numbers lie about 100 above batch A's largest: a
    1-byte number decodes only within 128 of the largest received (RFC 9000
    A.3), so they open against the committed state and fail the tag against 0."""
    rng = np.random.Generator(np.random.PCG64(8200 + 2 * suite + salamander))
    secrets, cids = [rng.bytes(32) for _ in range(2)], [rng.bytes(8) for _ in range(2)]
    wrap = lambda ps: [ol.salamander_write(PSK, rng.bytes(8), p)[0] for p in ps] if salamander else ps  # noqa: E731
    pns_a, pns_b = [990 + i for i in range(12)], [1100 + i for i in range(8)]
    a = short_packets(rng, suite, secrets, cids, pns_a, 2)
    b = short_packets(rng, suite, secrets, cids, pns_b, 1)
    dcid = rng.bytes(8)
    ipkt, ipno = initial(dcid, rng.bytes(5), b"", 1, 2, 2, 2, rng.bytes(1162))
    iprot = ol.quic_seal(*initial_keys(dcid, QUIC_SIDE_CLIENT), 2, ipkt, ipno, ol.AES128GCM)[0]
    stray = bytes([0x40]) + rng.bytes(8) + rng.bytes(40)
    wires_a = wrap([p for _, p in a[:5]] + [iprot] + [p for _, p in a[5:9]] + [stray] +
                   [p for _, p in a[9:]])
    idx_a = [0, 1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13]
    with sqobfs.QuicKeyring.from_secrets(ctx, [QuicSecret.of(s) for s in secrets], suite) as kr, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr0, \
            sqobfs.QuicCidMap(ctx, 2, 4, 8) as cmap, sqobfs.QuicCidMap(ctx, 2, 4, 8) as fresh:
        okr = okr0 if salamander else None
        for m in (cmap, fresh):
            m.update([(cids[0], 0), (cids[1], 1)])
        counts, res = route_and_open(ctx, cmap, kr, okr, wires_a, True)
        assert counts == [12, 1, 0, 0, 0, 1, 0, 0]
        assert res[QUIC_ROUTE_SHORT] == (idx_a, [p for p, _ in a], pns_a)
        assert res[QUIC_ROUTE_INITIAL] == ([5], [ipkt], [2])
        counts, res = route_and_open(ctx, cmap, kr, okr, wrap([p for _, p in b]), False)
        assert res[QUIC_ROUTE_SHORT] == (list(range(8)), [p for p, _ in b], pns_b)
        counts, res = route_and_open(ctx, fresh, kr, okr, wrap([p for _, p in b]), False)
        assert counts[0] == 8 and res[QUIC_ROUTE_SHORT][1] == [QUIC_EAUTH] * 8


def test_route_refusals(ctx):
    rng = np.random.Generator(np.random.PCG64(8300))
    for bad in ((0, 4, 8), (32769, 4, 8), (2, 0, 8), (2, 4, 0), (2, 4, 21)):
        with pytest.raises(sqobfs.SqError) as e:
            sqobfs.QuicCidMap(ctx, *bad)
        assert e.value.status == sqobfs.SQ_EINVAL
    cids = [rng.bytes(8) for _ in range(6)]
    wires = [bytes([0x40]) + c + rng.bytes(30) for c in cids]
    d_in, d_off, d_len, _, _ = place(wires)
    with sqobfs.QuicCidMap(ctx, 3, 4, 8) as cmap, sqobfs.Context(0) as ctx2, \
            sqobfs.Keyring(ctx, sqobfs.XPLUS, [PSK]) as xkr, \
            sqobfs.Keyring(ctx2, sqobfs.SALAMANDER, [PSK]) as other:
        cmap.update([(c, i % 3) for i, c in enumerate(cids[:4])])
        before = route(ctx, cmap, None, d_in, d_off, d_len)
        for ops in ([(cids[0], QUIC_CID_REMOVE), (cids[4], 1), (cids[5], 2)],  # 5 ids of 4
                    [(cids[0], QUIC_CID_REMOVE), (cids[1], 3)]):               # conn 3 of 3
            with pytest.raises(sqobfs.SqError) as e:
                cmap.update(ops)
            assert e.value.status == sqobfs.SQ_EINVAL
        with pytest.raises(sqobfs.SqError):
            cmap.reset_pn([3])
        after = route(ctx, cmap, None, d_in, d_off, d_len)
        for r in (before, after):
            assert r.cls.cpu().numpy().tolist() == [0, 0, 0, 0, 5, 5]
            assert r.conn.cpu().numpy().tolist() == [0, 1, 2, 0, QUIC_NOCONN, QUIC_NOCONN]
        for okr, bad in [(None, dict(pn_offset=1)), (None, dict(pn=1)), (None, dict(key_id=1)),
                         (xkr, {}), (other, {})]:
            with pytest.raises(sqobfs.SqError) as e:  # (route: count keeps its fill)
                route(ctx, cmap, okr, d_in, d_off, d_len, **bad)
            assert e.value.status == sqobfs.SQ_EINVAL
