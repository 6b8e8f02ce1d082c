"""sqobfs_quic_initial_open_salamander / _seal_salamander, bit-exact against
the CPU oracle alone: HKDF keys from hmac / hashlib, or_quic_seal / _open, and
the restated SalamanderPacketConn.WriteTo / ReadFrom around them."""
from __future__ import annotations

import types

import numpy as np
import pytest
import sqobfs
from sqobfs import QUIC_EAUTH, QUIC_EHEADER, QUIC_ESHORT, QUIC_SIDE_CLIENT, QUIC_SIDE_SERVER

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)
from test_gpu_quic_initial import GOLD, B, big_batch, initial, initial_keys

pytestmark = pytest.mark.gpu
FILL = 0xA5
# psk || salt8: in one BLAKE2b block, across the block boundary, in two blocks
PSKS = {n: bytes(range(1, 251))[:n] for n in (16, 124, 200)}


def wrap(psk, salts, dgrams):
    return [ol.salamander_write(psk, s, d)[0] for s, d in zip(salts, dgrams)]


def run(ctx, okr, seal, items, pns, side, odcid=None, inplace=False, salts=None, **bad):
    """One ragged batch, a slot per packet: seal reads at base + 8, open at
    base; both write at base, in place or into a second buffer of the same fill."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(dev)  # noqa: E731
    n = len(items)
    lens = np.array([len(p) for p in items], np.uint32)
    base = np.concatenate([[0], np.cumsum(lens + 8 + 24 + 5)]).astype(np.uint64)
    in_off = base[:-1] + (8 if seal else 0)
    data = np.full(int(base[-1]), FILL, np.uint8)
    for o, p in zip(in_off, items):
        data[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    d_in = t(data, np.uint8)
    d_out = d_in if inplace else t(np.full_like(data, FILL), np.uint8)
    r = dict(out_len=t(np.full(n, 7), np.uint32), pn_out=t(np.full(n, 7), np.uint64),
             pno=t(np.full(n, 7), np.uint16), consumed=t(np.full(n, 7), np.uint32))
    od = ol_ = None
    if odcid is not None:
        od = t(np.frombuffer(b"".join(c.ljust(20, b"\0") for c in odcid), np.uint8), np.uint8)
        ol_ = None if "half" in bad else t([len(c) for c in odcid], np.uint8)
    extra = {k: t(np.zeros(n), np.uint16) for k in bad if k in ("pn_offset", "key_id")}
    b = sqobfs.quic_batch(n, d_in, t(in_off, np.uint64), t(lens, np.uint32), d_out,
                          t(base[:-1], np.uint64), r["out_len"], extra.get("pn_offset"),
                          t(pns, np.uint64), extra.get("key_id"), r["pn_out"])
    d_salt = None if salts is None else t(np.frombuffer(b"".join(salts), np.uint8), np.uint8)
    torch.cuda.synchronize(dev)
    side = bad.get("bad_side", side)
    status = sqobfs.SQ_OK
    try:
        if seal:
            sqobfs.quic_initial_seal_salamander(ctx, okr, b, side, d_salt, od, ol_, r["pno"])
        else:
            sqobfs.quic_initial_open_salamander(ctx, okr, b, side, od, ol_, r["pno"],
                                                r["consumed"])
    except sqobfs.SqError as e:
        status = e.status
    ctx.sync()
    r = {k: v.cpu().numpy() for k, v in r.items()}
    r.update(status=status, buf=d_out.cpu().numpy(), base=base)
    r["out"] = [r["buf"][int(o):int(o) + int(m)].tobytes() if m < 2**20 else int(m)
                for o, m in zip(base, r["out_len"])]
    return r


@pytest.mark.parametrize("npsk", sorted(PSKS))
@pytest.mark.parametrize("side,given,inplace", [(QUIC_SIDE_CLIENT, 0, 0), (QUIC_SIDE_SERVER, 1, 1),
                                                (QUIC_SIDE_CLIENT, 1, 0), (QUIC_SIDE_SERVER, 0, 1)])
def test_seal_then_open(ctx, side, given, inplace, npsk):
    pkts, pnos, pns, largest, od, prot, dgram = big_batch(side, given)
    hdr = [pno + 1 + (p[0] & 3) for p, pno in zip(pkts, pnos)]  # where the payload's key starts
    assert {(h % 32) // 16 for h in hdr} == {0, 1} and any(h % 4 for h in hdr)
    assert max(pnos) > 300  # varints past byte 32, header blocks from memory
    rng = np.random.Generator(np.random.PCG64(7300 + npsk))
    salts = [rng.bytes(8) for _ in pkts]
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSKS[npsk]]) as okr:
        r = run(ctx, okr, True, pkts, pns, side, od, inplace, salts)
        assert r["out"] == wrap(PSKS[npsk], salts, prot) and r["pno"].tolist() == pnos
        wires = wrap(PSKS[npsk], salts, dgram)  # every third: 1-40 coalesced bytes
        r = run(ctx, okr, False, wires, largest, side, od, inplace)
    assert r["out"] == pkts and r["pn_out"].tolist() == pns and r["pno"].tolist() == pnos
    assert r["consumed"].tolist() == [len(p) for p in prot]
    for o, nxt, p, d in zip(r["base"], r["base"][1:], prot, dgram):
        o = int(o)  # the datagram's remainder at its own offset, nothing after it
        assert r["buf"][o + len(p):o + len(d)].tobytes() == d[len(p):]
        assert inplace or (r["buf"][o + len(d):int(nxt)] == FILL).all()


def test_rfc9001_a3(ctx):
    a1, a3 = GOLD["rfc9001_a1"], GOLD["rfc9001_a3"]
    pkt, prot = B(a3["header"] + a3["payload"]), B(a3["protected"])
    od, salt = [B(a1["dcid"])], [B("0011223344556677")]
    wire = wrap(PSKS[16], salt, [prot])
    plain, n = ol.salamander_read(PSKS[16], wire[0])
    assert plain[:n] == prot
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSKS[16]]) as okr:
        r = run(ctx, okr, True, [pkt], [a3["pn"]], QUIC_SIDE_SERVER, od, salts=salt)
        assert r["out"] == wire and r["pno"].tolist() == [a3["pn_offset"]]
        r = run(ctx, okr, False, wire, [0], QUIC_SIDE_SERVER, od)
    assert r["out"] == [pkt] and r["pn_out"].tolist() == [a3["pn"]]
    assert r["pno"].tolist() == [a3["pn_offset"]] and r["consumed"].tolist() == [len(prot)]


def test_rejects(ctx):
    rng = np.random.Generator(np.random.PCG64(7400))
    psk, dcid, scid, tok, side = PSKS[124], rng.bytes(8), rng.bytes(5), rng.bytes(300), 0
    mk = lambda **kw: initial(dcid, scid, tok, 2, 2, 5, 2, rng.bytes(120), **kw)  # noqa: E731
    seal = lambda pp: ol.quic_seal(*initial_keys(dcid, side), 5, pp[0], pp[1], ol.AES128GCM)[0]  # noqa: E731
    w = lambda d, k=psk: ol.salamander_write(k, rng.bytes(8), d)[0]  # noqa: E731
    flip = lambda d, k: d[:k] + bytes([d[k] ^ 0x10]) + d[k + 1:]  # noqa: E731
    pkt, pno = good = mk()
    prot = seal(good)
    anyerr = range(QUIC_EHEADER, 2**32)
    cases = [(w(prot), len(pkt)), (b"", QUIC_ESHORT), (w(prot)[:7], QUIC_ESHORT),
             (w(prot)[:8], QUIC_ESHORT),
             (w(seal(mk(first=0xE0))), QUIC_EHEADER), (w(seal(mk(first=0x40))), QUIC_EHEADER),
             (w(flip(prot, len(prot) - 1)), QUIC_EAUTH), (w(flip(prot, pno + 40)), QUIC_EAUTH),
             (flip(w(prot), 3), anyerr), (w(prot, PSKS[16]), anyerr),  # salt, PSK: garbage header
             (w(prot), len(pkt))]
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [psk]) as okr, \
            sqobfs.Keyring(ctx, sqobfs.XPLUS, [psk]) as xkr, sqobfs.Context(0) as ctx2, \
            sqobfs.Keyring(ctx2, sqobfs.SALAMANDER, [psk]) as other:
        r = run(ctx, okr, False, [c[0] for c in cases], [2] * len(cases), side)
        for got, (_, want) in zip(r["out_len"].tolist(), cases):
            assert got in want if isinstance(want, range) else got == want
        assert r["out"][0] == pkt and r["out"][-1] == pkt and r["consumed"].tolist()[1:10] == [7] * 9
        # seal: a Length field that disagrees with in_len, between two good packets
        salts = [rng.bytes(8) for _ in range(3)]
        r = run(ctx, okr, True, [pkt, mk(length=139)[0], pkt], [5] * 3, side, salts=salts)
        assert r["out_len"].tolist() == [len(prot) + 8, QUIC_EHEADER, len(prot) + 8]
        assert [r["out"][0], r["out"][2]] == wrap(psk, salts[::2], [prot] * 2)
        # refused on the host, before anything is launched: the outputs keep their fill
        none = types.SimpleNamespace(handle=None)
        for is_seal, item in ((False, w(prot)), (True, pkt)):
            for kr, bad in [(okr, dict(pn_offset=1)), (okr, dict(key_id=1)), (okr, dict(bad_side=2)),
                            (okr, dict(half=1)), (none, {}), (xkr, {}), (other, {})] + \
                    ([(okr, dict(nosalt=1))] if is_seal else []):
                r = run(ctx, kr, is_seal, [item], [2], side, [dcid], False,
                        None if "nosalt" in bad or not is_seal else salts[:1], **bad)
                assert r["status"] == sqobfs.SQ_EINVAL, (is_seal, bad)
                assert r["out_len"].tolist() == [7] and (r["buf"] == FILL).all()
