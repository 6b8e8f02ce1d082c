"""QUIC v1 Initial packets opened and sealed with keys derived per packet on
the GPU (sqobfs_quic_initial_open / _seal).  The reference is independent of
the kernels: keys by HKDF from hmac / hashlib (RFC 9001 5.2), packets from the
CPU oracle's AES-128-GCM seal / open at the pn_offset the test built."""
from __future__ import annotations

import functools
import hashlib
import hmac
import json
import struct

import numpy as np
import pytest
import sqobfs
from sqobfs import QUIC_EAUTH, QUIC_EHEADER, QUIC_ESHORT, QUIC_SIDE_CLIENT, QUIC_SIDE_SERVER

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
B = bytes.fromhex
GOLD = json.load(open(ol.REPO + "/tests/golden/quic_gcm.json"))
SALT = B(GOLD["rfc9001_a1"]["initial_salt"])


def expand_label(secret, label, n):
    info = struct.pack(">HB", n, 6 + len(label)) + b"tls13 " + label + b"\0"
    return hmac.new(secret, info + b"\x01", hashlib.sha256).digest()[:n]


def initial_keys(dcid, side):
    sec = expand_label(hmac.new(SALT, dcid, hashlib.sha256).digest(),
                       b"server in" if side == QUIC_SIDE_SERVER else b"client in", 32)
    return (expand_label(sec, b"quic key", 16), expand_label(sec, b"quic iv", 12),
            expand_label(sec, b"quic hp", 16))


def varint(v, nbytes):
    return (v | ((nbytes.bit_length() - 1) << (8 * nbytes - 2))).to_bytes(nbytes, "big")


def initial(dcid, scid, token, tok_vl, len_vl, pn, pn_len, payload, first=0xC0, version=1,
            dlen=None, length=None):
    """(unprotected header || payload, pn_offset)."""
    length = pn_len + len(payload) + 16 if length is None else length
    h = bytes([first | (pn_len - 1)]) + struct.pack(">IB", version, len(dcid) if dlen is None
                                                    else dlen) + dcid + bytes([len(scid)]) + \
        scid + varint(len(token), tok_vl) + token + varint(length, len_vl)
    return h + (pn % 256**pn_len).to_bytes(pn_len, "big") + payload, len(h)


def launch(ctx, fn, pkts, pns, side, odcid=None, inplace=False, odlen=None, **bad):
    """One batch at ragged offsets; odcid: per-packet DCIDs or None; bad:
    quic_batch fields that must be rejected.  Returns numpy results."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(dev)  # noqa: E731
    n = len(pkts)
    lens = np.array([len(p) for p in pkts], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens + 16 + 5)]).astype(np.uint64)
    data = np.full(int(off[-1]), 0xA5, np.uint8)
    for o, p in zip(off, pkts):
        data[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    d_in = t(data, np.uint8)
    d_out = d_in if inplace else t(np.full_like(data, 0xA5), np.uint8)
    d_off, d_len, d_pn = t(off[:-1], np.uint64), t(lens, np.uint32), t(pns, np.uint64)
    r = dict(out_len=t(np.full(n, 7), np.uint32), pn_out=t(np.full(n, 7), np.uint64),
             pno=t(np.full(n, 7), np.uint16), consumed=t(np.full(n, 7), np.uint32))
    od = ol_ = None
    if odcid is not None:
        od = t(np.frombuffer(b"".join(c.ljust(20, b"\0") for c in odcid), np.uint8), np.uint8)
        ol_ = t([len(c) for c in odcid] if odlen is None else odlen, np.uint8)
    extra = {k: t(np.zeros(n), np.uint16) for k in bad if k in ("pn_offset", "key_id")}
    b = sqobfs.quic_batch(n, d_in, d_off, d_len, d_out, d_off, r["out_len"],
                          extra.get("pn_offset"), d_pn, extra.get("key_id"), r["pn_out"])
    torch.cuda.synchronize(dev)
    args = (ctx, b, bad.get("bad_side", side), od, None if "half" in bad else ol_, r["pno"])
    status = sqobfs.SQ_OK
    try:
        fn(*args, *([r["consumed"]] if fn is sqobfs.quic_initial_open else []))
    except sqobfs.SqError as e:
        status = e.status
    ctx.sync()
    r = {k: v.cpu().numpy() for k, v in r.items()}
    r["status"] = status
    r["buf"], r["off"] = d_out.cpu().numpy(), off
    r["out"] = [r["buf"][int(o):int(o) + int(m)].tobytes() if m < 2**20 else int(m)
                for o, m in zip(off, r["out_len"])]
    return r


def test_rfc9001_vectors(ctx):
    a1, a3 = GOLD["rfc9001_a1"], GOLD["rfc9001_a3"]
    for side, name in ((QUIC_SIDE_CLIENT, "client"), (QUIC_SIDE_SERVER, "server")):
        assert [x.hex() for x in initial_keys(B(a1["dcid"]), side)] == \
            [a1[name][k] for k in ("key", "iv", "hp")]
    pkt, prot = B(a3["header"] + a3["payload"]), B(a3["protected"])
    od = [B(a1["dcid"])]
    r = launch(ctx, sqobfs.quic_initial_seal, [pkt], [a3["pn"]], QUIC_SIDE_SERVER, od)
    assert r["out"] == [prot] and r["pno"].tolist() == [a3["pn_offset"]]
    r = launch(ctx, sqobfs.quic_initial_open, [prot], [0], QUIC_SIDE_SERVER, od)
    assert r["out"] == [pkt] and r["pn_out"].tolist() == [a3["pn"]]
    assert r["pno"].tolist() == [a3["pn_offset"]] and r["consumed"].tolist() == [len(prot)]


@functools.lru_cache(maxsize=None)
def big_batch(side, given):
    """150 Initials over every header and payload shape, with the oracle's
    protected form; given: keys from a DCID that is not the packet's own."""
    rng = np.random.Generator(np.random.PCG64(7100 + 2 * side + given))
    pay = [None, 15, 16, 17, 63, 64, 65, 1162, 1452]
    pkts, pnos, pns, largest, kd, prot, nblk = [], [], [], [], [], [], set()
    for i in range(150):
        pn_len, tl = 1 + (i // 4) % 4, [0, 1, 63, 64, 300][i % 5]
        plen = pay[i % 9] if pay[i % 9] is not None else 4 - pn_len  # None: the least sampleable
        # the truncated number sits just past a window boundary of largest + 1
        pn = (int(rng.integers(1, 2**20)) << (8 * pn_len)) + i % 3
        vl = [1, 2, 4][i % 3]
        pkt, pno = initial(rng.bytes([0, 1, 8, 20][i % 4]), rng.bytes([0, 20][(i // 2) % 2]),
                           rng.bytes(tl), 2 if tl >= 64 else 1 + i % 2,
                           2 if vl == 1 and pn_len + plen + 16 >= 64 else vl, pn, pn_len,
                           rng.bytes(plen))
        dcid = rng.bytes(int(rng.integers(0, 21))) if given else pkt[6:6 + pkt[5]]
        p, rc = ol.quic_seal(*initial_keys(dcid, side), pn, pkt, pno, ol.AES128GCM)
        assert rc == len(pkt) + 16
        back, rc, got_pn = ol.quic_open(*initial_keys(dcid, side), pn - 3, p, pno, ol.AES128GCM)
        assert (back[:len(pkt)], got_pn) == (pkt, pn)
        nblk.add(((pno + pn_len + 15) // 16 + (plen + 15) // 16 + 1) % 4)
        for lst, v in zip((pkts, pnos, pns, largest, kd, prot), (pkt, pno, pn, pn - 3, dcid, p)):
            lst.append(v)
    assert nblk == {0, 1, 2, 3}
    dgram = [p + (rng.bytes(1 + i % 40) if i % 3 == 0 else b"") for i, p in enumerate(prot)]
    return pkts, pnos, pns, largest, kd if given else None, prot, dgram


@pytest.mark.parametrize("side,given,inplace", [(QUIC_SIDE_CLIENT, 0, 0), (QUIC_SIDE_SERVER, 1, 1),
                                                (QUIC_SIDE_CLIENT, 1, 0), (QUIC_SIDE_SERVER, 0, 1)])
def test_seal_then_open(ctx, side, given, inplace):
    pkts, pnos, pns, largest, od, prot, dgram = big_batch(side, given)
    r = launch(ctx, sqobfs.quic_initial_seal, pkts, pns, side, od, inplace)
    assert r["out"] == prot and r["pno"].tolist() == pnos
    r = launch(ctx, sqobfs.quic_initial_open, dgram, largest, side, od, inplace)
    assert r["out"] == pkts and r["out_len"].tolist() == [len(p) for p in pkts]
    assert r["pn_out"].tolist() == pns and r["pno"].tolist() == pnos
    assert r["consumed"].tolist() == [len(p) for p in prot]
    if not inplace:  # nothing past out_len: not the tag's room, not a coalesced packet
        for o, m, nxt in zip(r["off"], r["out_len"], r["off"][1:]):
            assert (r["buf"][int(o) + int(m):int(nxt)] == 0xA5).all()


def test_rejects(ctx):
    rng = np.random.Generator(np.random.PCG64(7200))
    dcid, scid, tok, side = rng.bytes(8), rng.bytes(5), rng.bytes(300), QUIC_SIDE_CLIENT
    mk = lambda **kw: initial(dcid, scid, tok, 2, 2, 5, 2, rng.bytes(120), **kw)  # noqa: E731
    seal = lambda pp: ol.quic_seal(*initial_keys(dcid, side), 5, pp[0], pp[1], ol.AES128GCM)[0]  # noqa: E731
    pkt, pno = good = mk()
    prot = seal(good)
    flip = lambda k: prot[:k] + bytes([prot[k] ^ 0x10]) + prot[k + 1:]  # noqa: E731
    cases = [(prot, len(pkt)),
             (seal(mk(first=0x40)), QUIC_EHEADER),                # a short header
             (seal(mk(version=0x6B3343CF)), QUIC_EHEADER),        # QUIC v2
             (seal(mk(version=0)), QUIC_EHEADER),
             (seal(mk(first=0xE0)), QUIC_EHEADER),                # Handshake
             (seal(mk(dlen=21)), QUIC_EHEADER),
             (prot, QUIC_EHEADER),                                # given odcid_len 21
             (prot[:100], QUIC_ESHORT),                           # cut inside the token
             (prot[:-1], QUIC_ESHORT),                            # Length past in_len
             (seal(mk(length=19))[:pno + 19], QUIC_ESHORT),       # too short to sample
             (flip(len(prot) - 1), QUIC_EAUTH), (flip(pno + 40), QUIC_EAUTH),
             (flip(40), QUIC_EAUTH), (flip(7), QUIC_EAUTH),       # tag, body, token, DCID
             (prot, len(pkt))]
    dg, want = [c[0] for c in cases], [c[1] for c in cases]
    odlen = [21 if i == 6 else 8 for i in range(len(dg))]
    r = launch(ctx, sqobfs.quic_initial_open, dg, [2] * len(dg), side, [dcid] * len(dg),
               odlen=odlen)
    assert r["out_len"].tolist() == want
    assert r["out"][0] == pkt and r["out"][-1] == pkt
    assert r["pn_out"].tolist()[0] == 5 and r["consumed"].tolist()[1:10] == [7] * 9
    # seal: a Length field that disagrees with in_len, between two good packets
    r = launch(ctx, sqobfs.quic_initial_seal, [pkt, mk(length=139)[0], pkt], [5] * 3, side)
    assert r["out_len"].tolist() == [len(prot), QUIC_EHEADER, len(prot)]
    assert r["out"][0] == prot and r["out"][2] == prot
    # refused on the host, before anything is launched: the outputs keep their fill
    for fn in (sqobfs.quic_initial_open, sqobfs.quic_initial_seal):
        for bad in (dict(pn_offset=1), dict(key_id=1), dict(bad_side=2), dict(half=1)):
            r = launch(ctx, fn, [prot], [2], side, [dcid], **bad)
            assert r["status"] == sqobfs.SQ_EINVAL, bad
            assert r["out_len"].tolist() == [7] and (r["buf"] == 0xA5).all()
