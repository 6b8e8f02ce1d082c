"""sqobfs_quic_key_phase_salamander, all three suites: datagrams sealed under
four generations' keys (HKDF from hmac / hashlib) resolve to the entry that
sealed them, and sqobfs_quic_open_salamander with that output opens them."""
from __future__ import annotations

import struct

import numpy as np
import pytest
import sqobfs
from sqobfs import QuicKeyring, QuicSecret

import oracle_lib as ol
from test_gpu_quic import ctx  # noqa: F401  (fixture)
from test_gpu_quic_keys import SUITES, gen_key, launch
from test_gpu_quic_obfs import PSK, _seal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("suite,h,kl", SUITES, ids=["chacha20", "aes128", "aes256"])
def test_key_phase_salamander(ctx, suite, h, kl):
    import torch
    rng = np.random.Generator(np.random.PCG64(960 + suite))
    secrets = [rng.bytes(h().digest_size) for _ in range(2)]
    # connection 0 holds generations 0 and 1, connection 1 (rolled twice) 2 and 3
    keys = [gen_key(h, kl, secrets[e // 2], e) for e in range(4)]
    # DCIDs of 0, 8 and 20 bytes: the sample at pn_offset + 4 = 5, 13 and 25
    # crosses the key's 16- and 32-byte boundaries
    sealed_with = [e for e in range(4) for _ in range(6)] + [2]
    dls = [[0, 8, 20][i % 3] for i in range(24)] + [8]
    pns = rng.integers(1, 2**30, len(dls))
    pkts = [bytes([0x43 | ((e & 1) << 2)]) + rng.bytes(dl) + struct.pack(">I", int(pn)) +
            rng.bytes(int(rng.integers(20, 300))) for e, dl, pn in zip(sealed_with, dls, pns)]
    pkts[-1] = bytes([0xC3]) + pkts[-1][1:]  # a long header: no key phase
    pnos = [1 + dl for dl in dls]
    salts = [rng.bytes(8) for _ in pkts]
    with sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr, \
            QuicKeyring.from_secrets(ctx, [QuicSecret.of(s) for s in secrets], suite) as kr:
        kr.rekey([1]), kr.rekey([1])
        out, oo, olen, _ = _seal(ctx, keys, okr, pkts, pnos, pns, salts, sealed_with, suite=suite)
        wires = [out[int(o):int(o) + int(m)].tobytes() for o, m in zip(oo, olen)]
        assert [len(w) for w in wires] == [len(p) + 24 for p in pkts]
        # too short to sample, shorter than the salt, an id out of range: key_id is kept
        wires += [ol.salamander_write(PSK, salts[0], rng.bytes(9 + 19))[0], b"abc", wires[0]]
        given = [e & ~1 for e in sealed_with] + [3, 1, 9]
        pnos += [9, 9, pnos[0]]
        largest = np.concatenate([pns - 1, [0, 0, 0]])
        b, d, _ = launch(ctx, None, kr, wires, largest, given, pnos)  # (builds the batch only)
        ids = torch.from_numpy(np.full(len(wires), 0xFFFF, np.uint16)).to(d["in_"].device)
        wire = d["in_"].cpu().numpy().copy()
        sqobfs.quic_key_phase_salamander(ctx, kr, okr, b, ids)
        ctx.sync()
        assert ids.cpu().numpy().tolist() == sealed_with + [3, 1, 9]
        assert np.array_equal(d["in_"].cpu().numpy(), wire), "the input is not modified"
        b, d, _ = launch(ctx, None, kr, wires, largest, ids.cpu().numpy(), pnos)
        sqobfs.quic_open_salamander(ctx, kr, okr, b)
        ctx.sync()
        with sqobfs.Keyring(ctx, sqobfs.XPLUS, [PSK]) as xkr, pytest.raises(sqobfs.SqError):
            sqobfs.quic_key_phase_salamander(ctx, kr, xkr, b, ids)  # refused on the host
    got, m, off = d["out"].cpu().numpy(), d["out_len"].cpu().numpy(), d["off"].cpu().numpy()
    assert m.tolist()[:len(pkts)] == [len(p) for p in pkts]
    assert [got[int(o):int(o) + len(p)].tobytes() for o, p in zip(off, pkts)] == pkts
    assert d["pn_out"].cpu().numpy().tolist()[:len(pkts)] == pns.tolist()
    assert m[len(pkts)] == sqobfs.QUIC_ESHORT and m[len(pkts) + 1] == sqobfs.QUIC_ESHORT
