#!/usr/bin/env python3
"""Measures QUIC Initial protection with per-packet keys.

One process, repetitions alternating between the routes, median and spread:
  new      sqobfs_quic_initial_open / _seal of N client Initials, distinct DCIDs
  keyring  the same open on the keyring interface, end to end: HKDF per DCID
           on the host (hmac / hashlib), a keyring of N AES-128-GCM entries,
           then sqobfs_quic_open with key ids
  onekey   sqobfs_quic_open of packets of the same sizes under one key: the
           floor that per-packet keys are paid over
The same batch wrapped in the Salamander layer:
  two-step sqobfs.launch de-obfuscates into a scratch buffer, then
           sqobfs_quic_initial_open; seal in the reverse order
  fused    sqobfs_quic_initial_open_salamander / _seal_salamander
and, `--phase`, sqobfs_quic_key_phase_salamander against the
sqobfs_quic_open_salamander it precedes, per suite, on N short-header packets.
Prints one JSON line and writes it to --out.  `--only new` / `--only fused`
runs that route alone (under a kernel trace it gives the split between the
kernels).
"""
from __future__ import annotations

import argparse
import hashlib
import hmac
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sing-quic_amd"))
import sqobfs  # noqa: E402
from sqobfs import QuicKey, QuicKeyring  # noqa: E402

SALT = bytes.fromhex("38762cf7f55934b34d179ae6a4c80cadccbb7f0a")  # RFC 9001 5.2
DGRAM, PNO, PN_LEN, SLOT = 1200, 26, 2, 1216


def expand_label(secret, label, n):
    info = struct.pack(">HB", n, 6 + len(label)) + b"tls13 " + label + b"\0"
    return hmac.new(secret, info + b"\x01", hashlib.sha256).digest()[:n]


def client_keys(dcid):
    sec = expand_label(hmac.new(SALT, dcid, hashlib.sha256).digest(), b"client in", 32)
    return QuicKey.of(expand_label(sec, b"quic key", 16), expand_label(sec, b"quic iv", 12),
                      expand_label(sec, b"quic hp", 16))


def spread(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 1), "min_us": round(min(xs) * 1e6, 1),
            "max_us": round(max(xs) * 1e6, 1), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65535)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--keyring-reps", type=int, default=3)
    ap.add_argument("--only", choices=["new", "fused"], default=None)
    ap.add_argument("--phase", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the CPU"
    dev = torch.device("cuda", 0)
    n = a.n
    rng = np.random.Generator(np.random.PCG64(94))
    # c1 | version 1 | 8-byte DCID | 8-byte SCID | no token | Length (2 bytes) | pn (2 bytes)
    plain = np.zeros((n, SLOT), np.uint8)
    plain[:, :DGRAM - 16] = rng.integers(0, 256, (n, DGRAM - 16), dtype=np.uint8)
    dcids = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    dcids[:, :4] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)  # distinct
    plain[:, 0], plain[:, 1:5], plain[:, 5], plain[:, 6:14] = 0xC1, [0, 0, 0, 1], 8, dcids
    plain[:, 14], plain[:, 23] = 8, 0
    plain[:, 24:26] = list(struct.pack(">H", 0x4000 | (DGRAM - PNO)))
    pns = np.arange(n, dtype=np.uint64) % 60000
    plain[:, 26], plain[:, 27] = pns >> 8, pns & 255
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    off = t(np.arange(n, dtype=np.uint64) * SLOT)
    d_plain, d_wire, d_back = t(plain.reshape(-1)), t(np.zeros(n * SLOT, np.uint8)), \
        t(np.zeros(n * SLOT, np.uint8))
    len_p, len_w = t(np.full(n, DGRAM - 16, np.uint32)), t(np.full(n, DGRAM, np.uint32))
    d_pn, d_largest = t(pns), t(np.maximum(pns, 1) - 1)
    out_len, pn_out = t(np.zeros(n, np.uint32)), t(np.zeros(n, np.uint64))
    pno = t(np.full(n, PNO, np.uint16))
    kid = t(np.arange(n, dtype=np.uint16))
    res = {"n": n, "datagram_bytes": DGRAM}
    with sqobfs.Context(0) as ctx:
        def timed(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        b_seal = sqobfs.quic_batch(n, d_plain, off, len_p, d_wire, off, out_len, None, d_pn)
        b_open = sqobfs.quic_batch(n, d_wire, off, len_w, d_back, off, out_len, None, d_largest,
                                   None, pn_out)
        new_seal = lambda: sqobfs.quic_initial_seal(ctx, b_seal, sqobfs.QUIC_SIDE_CLIENT)  # noqa: E731
        new_open = lambda: sqobfs.quic_initial_open(ctx, b_open, sqobfs.QUIC_SIDE_CLIENT)  # noqa: E731
        timed(new_seal)
        assert bool((out_len == DGRAM).all())
        timed(new_open)
        assert bool((out_len == DGRAM - 16).all()) and bool((pn_out == d_pn).all())
        want = d_plain.view(n, SLOT)[:, :DGRAM - 16]
        assert torch.equal(d_back.view(n, SLOT)[:, :DGRAM - 16], want)
        if a.only == "new":
            for _ in range(a.reps):
                timed(new_seal), timed(new_open)
            return
        # the same batch under the Salamander layer: datagrams of DGRAM + 8 bytes
        okr = sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [b"sing-quic-mi355x-bench-psk"])
        d_salt = t(rng.integers(0, 256, n * 8, dtype=np.uint8))
        d_ow, d_ow2 = t(np.zeros(n * SLOT, np.uint8)), t(np.zeros(n * SLOT, np.uint8))
        len_ow, len_tmp = t(np.full(n, DGRAM + 8, np.uint32)), t(np.zeros(n, np.uint32))
        bf_seal = sqobfs.quic_batch(n, d_plain, off, len_p, d_ow, off, out_len, None, d_pn)
        bf_open = sqobfs.quic_batch(n, d_ow, off, len_ow, d_back, off, out_len, None, d_largest,
                                    None, pn_out)
        b_obf = sqobfs.make_batch(n, d_wire, off, len_w, d_ow2, off, len_tmp, salt=d_salt)
        b_deo = sqobfs.make_batch(n, d_ow, off, len_ow, d_wire, off, len_tmp)
        side = sqobfs.QUIC_SIDE_CLIENT
        fused_seal = lambda: sqobfs.quic_initial_seal_salamander(ctx, okr, bf_seal, side, d_salt)  # noqa: E731
        fused_open = lambda: sqobfs.quic_initial_open_salamander(ctx, okr, bf_open, side)  # noqa: E731

        def two_seal():  # d_plain -> d_wire -> d_ow2
            new_seal()
            sqobfs.launch(ctx, okr, sqobfs.OBFUSCATE, b_obf)

        def two_open():  # d_ow -> d_wire -> d_back
            sqobfs.launch(ctx, okr, sqobfs.DEOBFUSCATE, b_deo)
            new_open()

        timed(fused_seal), timed(two_seal)
        assert bool((out_len == DGRAM).all()) and torch.equal(d_ow, d_ow2), "the routes differ"
        for fn in (fused_open, two_open):
            d_back.zero_()
            timed(fn)
            assert bool((out_len == DGRAM - 16).all()) and bool((pn_out == d_pn).all())
            assert torch.equal(d_back.view(n, SLOT)[:, :DGRAM - 16], want)
        if a.only == "fused":
            for _ in range(a.reps):
                timed(fused_seal), timed(fused_open)
            return
        TS = {"fused_open": [], "two_step_open": [], "fused_seal": [], "two_step_seal": []}
        for r in range(a.reps):
            TS["fused_open"].append(timed(fused_open))
            TS["two_step_open"].append(timed(two_open))
            TS["fused_seal"].append(timed(fused_seal))
            TS["two_step_seal"].append(timed(two_seal))
        res.update({k: spread(v) for k, v in TS.items()})
        if a.phase:  # two generations of one connection, random phases, pn_offset 9
            ph = rng.integers(0, 2, n).astype(np.uint16)
            plain[:, 0], plain[:, 9:13] = 0x43 | (ph << 2), 0
            d_short, d_ph, pno9 = t(plain.reshape(-1)), t(ph), t(np.full(n, 9, np.uint16))
            ids, zero = t(np.zeros(n, np.uint16)), t(np.zeros(n, np.uint64))
            for name, suite, hl in (("chacha20", sqobfs.QUIC_CHACHA20_POLY1305, 32),
                                    ("aes128", sqobfs.QUIC_AES_128_GCM, 32),
                                    ("aes256", sqobfs.QUIC_AES_256_GCM, 48)):
                with QuicKeyring.from_secrets(ctx, [sqobfs.QuicSecret.of(bytes(range(hl)))],
                                              suite) as kr:
                    bs = sqobfs.quic_batch(n, d_short, off, len_p, d_ow, off, out_len, pno9, zero,
                                           d_ph)
                    bo = sqobfs.quic_batch(n, d_ow, off, len_ow, d_back, off, out_len, pno9, zero,
                                           None, pn_out)
                    bo2 = sqobfs.quic_batch(n, d_ow, off, len_ow, d_back, off, out_len, pno9, zero,
                                            ids, pn_out)
                    sqobfs.quic_seal_salamander(ctx, kr, okr, bs, d_salt)
                    resolve = lambda: sqobfs.quic_key_phase_salamander(ctx, kr, okr, bo, ids)  # noqa: E731
                    opn = lambda: sqobfs.quic_open_salamander(ctx, kr, okr, bo2)  # noqa: E731
                    timed(resolve), timed(opn)
                    assert torch.equal(ids, d_ph) and bool((out_len == DGRAM - 16).all())
                    tp, to = [], []
                    for _ in range(a.reps):
                        tp.append(timed(resolve))
                        to.append(timed(opn))
                    res["phase_" + name] = {"key_phase_salamander": spread(tp),
                                            "open_salamander": spread(to)}
        okr.close()
        # the keyring route, end to end (also the warm-up of its kernels)
        b_kr = sqobfs.quic_batch(n, d_wire, off, len_w, d_back, off, out_len, pno, d_largest, kid,
                                 pn_out)

        def keyring_route(parts):
            t0 = time.perf_counter()
            keys = [client_keys(bytes(d)) for d in dcids]
            t1 = time.perf_counter()
            with QuicKeyring(ctx, keys, sqobfs.QUIC_AES_128_GCM) as kr:
                ctx.sync()
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                sqobfs.quic_open(ctx, kr, b_kr)
                ctx.sync()
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
            parts.append((t1 - t0, t2 - t1, t3 - t2))

        one = QuicKeyring(ctx, [client_keys(bytes(dcids[0]))], sqobfs.QUIC_AES_128_GCM)
        d_wire1 = t(np.zeros(n * SLOT, np.uint8))
        b_seal1 = sqobfs.quic_batch(n, d_plain, off, len_p, d_wire1, off, out_len, pno, d_pn)
        b_open1 = sqobfs.quic_batch(n, d_wire1, off, len_w, d_back, off, out_len, pno, d_largest,
                                    None, pn_out)
        timed(lambda: sqobfs.quic_seal(ctx, one, b_seal1))
        timed(lambda: sqobfs.quic_open(ctx, one, b_open1))
        assert bool((out_len == DGRAM - 16).all())
        T = {"new_open": [], "new_seal": [], "onekey_open": [], "onekey_seal": []}
        parts = []
        for r in range(a.reps):
            T["new_open"].append(timed(new_open))
            T["onekey_open"].append(timed(lambda: sqobfs.quic_open(ctx, one, b_open1)))
            T["new_seal"].append(timed(new_seal))
            T["onekey_seal"].append(timed(lambda: sqobfs.quic_seal(ctx, one, b_seal1)))
            if r < a.keyring_reps:
                d_back.zero_()
                keyring_route(parts)
                assert bool((out_len == DGRAM - 16).all())
                assert torch.equal(d_back.view(n, SLOT)[:, :DGRAM - 16], want)
        one.close()
        res.update({k: spread(v) for k, v in T.items()})
        res["keyring_open_end_to_end"] = spread([sum(p) for p in parts])
        res["keyring_parts"] = {"host_hkdf": spread([p[0] for p in parts]),
                                "keyring_create": spread([p[1] for p in parts]),
                                "open_with_key_ids": spread([p[2] for p in parts])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
