#!/usr/bin/env python3
"""Measures stateless-reset building and matching against
the router and the key-phase resolver, which read the same head bytes and,
fused, derive the same BLAKE2b key.

One process; per batch size and wire form (plain, under Salamander) the calls
alternate within each repetition; median and min-max:
  reset        sqobfs_quic_reset(_salamander), 42-byte resets
  match        sqobfs_quic_reset_match(_salamander) on the same datagrams (their
               last 16 bytes are AEAD tags: every probe misses)
  match_hits   the same call on the resets just built (every probe hits)
  route        sqobfs_quic_route(_salamander) on the same datagrams
  key_phase    sqobfs_quic_key_phase(_salamander) on the same datagrams
The batch: N sealed short-header datagrams of 1,350 bytes (+ 8 under
Salamander) over 1,024 connections with 8-byte connection ids, AES-128-GCM.
The token table holds one token per connection id (HMAC of the id under the
reset key, as a quic-go peer advertises them).  Before timing, a sample of the
resets is compared with Python's hmac and the CPU oracle's ChaCha20 and
Salamander, and every reset must match its connection.  Prints one JSON line
and writes it to --out.
"""
from __future__ import annotations

import argparse
import hashlib
import hmac
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sing-quic_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import sqobfs  # noqa: E402

DGRAM, SLOT, CONNS, PNO, CID, RLEN, RSLOT, SAMPLE = 1350, 1376, 1024, 9, 8, 42, 64, 512
PSK = b"sing-quic-mi355x-bench-psk"
KEY, SKEY = bytes(range(32)), bytes(range(100, 132))
CALLS = ["reset", "match", "match_hits", "route", "key_phase"]


def spread(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 1), "min_us": round(min(xs) * 1e6, 1),
            "max_us": round(max(xs) * 1e6, 1), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65535, 1 << 20])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=CALLS, default=None, help="that call alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import oracle_lib as ol
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the CPU"
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(946))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    cids = rng.integers(0, 256, (CONNS, CID), dtype=np.uint8)
    cids[:, :2] = np.arange(CONNS, dtype=">u2").view(np.uint8).reshape(CONNS, 2)  # distinct
    tokens = [hmac.new(KEY, bytes(c), hashlib.sha256).digest()[:16] for c in cids]
    res = {"datagram_bytes": DGRAM, "conns": CONNS, "reset_bytes": RLEN}
    with sqobfs.Context(0) as ctx, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr, \
            sqobfs.QuicKeyring.from_secrets(
                ctx, [sqobfs.QuicSecret.of(rng.bytes(32)) for _ in range(CONNS)],
                sqobfs.QUIC_AES_128_GCM) as kr, \
            sqobfs.QuicCidMap(ctx, CONNS, 2 * CONNS, CID) as cmap:
        cmap.update([(bytes(c), i) for i, c in enumerate(cids)])
        cmap.update_reset([(tok, i) for i, tok in enumerate(tokens)])

        def timed(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        for n in a.n:
            conn = rng.integers(0, CONNS, n)
            plain = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device=dev)
            plain[:, 0] = 0x43
            plain[:, 1:1 + CID] = t(cids[conn])
            off = t(np.arange(n, dtype=np.uint64) * SLOT)
            r_off = t(np.arange(n, dtype=np.uint64) * RSLOT)
            out_len, r_len = t(np.zeros(n, np.uint32)), t(np.zeros(n, np.uint32))
            ids, pno = t(np.zeros(n, np.uint16)), t(np.full(n, PNO, np.uint16))
            kid0, zero = t((2 * conn).astype(np.uint16)), t(np.zeros(n, np.uint64))
            conn_out, hits = t(np.zeros(n, np.uint32)), t(np.zeros(1, np.uint32))
            salts = rng.integers(0, 256, (n, 8), dtype=np.uint8)
            d_salt = t(salts.reshape(-1))
            for form in ("plain", "salamander"):
                ob = form == "salamander"
                o = okr if ob else None
                wire = torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
                r_out = torch.zeros(n * RSLOT, dtype=torch.uint8, device=dev)
                len_w = t(np.full(n, DGRAM + 8 * ob, np.uint32))
                bs = sqobfs.quic_batch(n, plain.view(-1), off, t(np.full(n, DGRAM - 16, np.uint32)),
                                       wire, off, out_len, pno, t(np.arange(n, dtype=np.uint64)), kid0)
                if ob:
                    sqobfs.quic_seal_salamander(ctx, kr, okr, bs,
                                                t(rng.integers(0, 256, n * 8, dtype=np.uint8)))
                else:
                    sqobfs.quic_seal(ctx, kr, bs)
                ctx.sync()
                routed = sqobfs.QuicRouted(n, dev, out_off=False)
                b_in = sqobfs.quic_batch(n, wire, off, len_w, None, None, None, None, None)
                b_rst = sqobfs.quic_batch(n, wire, off, len_w, r_out, r_off, r_len, None, None)
                b_hit = sqobfs.quic_batch(n, r_out, r_off, r_len, None, None, None, None, None)
                b_res = sqobfs.quic_batch(n, wire, off, len_w, None, None, None, pno, zero, kid0)
                calls = {
                    "reset": lambda: sqobfs.quic_reset(ctx, b_rst, KEY, CID, RLEN, o, d_salt),
                    "match": lambda: sqobfs.quic_reset_match(ctx, cmap, b_in, conn_out, hits, o),
                    "match_hits": lambda: sqobfs.quic_reset_match(ctx, cmap, b_hit, conn_out, hits, o),
                    "route": (lambda: sqobfs.quic_route_salamander(ctx, cmap, okr, b_in, routed)) if ob
                    else (lambda: sqobfs.quic_route(ctx, cmap, b_in, routed)),
                    "key_phase": (lambda: sqobfs.quic_key_phase_salamander(ctx, kr, okr, b_res, ids))
                    if ob else (lambda: sqobfs.quic_key_phase(ctx, kr, b_res, ids)),
                }
                # warm-up, and the results are right
                ctx.salt_key(SKEY, 5)
                timed(calls["reset"])
                assert bool((r_len == RLEN + 8 * ob).all())
                got = r_out.view(n, RSLOT)[:SAMPLE].cpu().numpy()
                for i in range(min(n, SAMPLE)):
                    fill = ol.chacha20_stream(SKEY, b"sqsr" + (5).to_bytes(8, "little"), i, RLEN - 16)
                    w = bytes([(fill[0] & 0x3F) | 0x40]) + fill[1:] + tokens[conn[i]]
                    w = ol.salamander_write(PSK, salts[i].tobytes(), w)[0] if ob else w
                    assert got[i, :len(w)].tobytes() == w, (form, i)
                hits.zero_()
                timed(calls["match_hits"])
                assert np.array_equal(conn_out.cpu().numpy(), conn) and int(hits.cpu()[0]) == n
                hits.zero_()
                timed(calls["match"])
                assert bool((conn_out == sqobfs.QUIC_NOCONN).all()) and int(hits.cpu()[0]) == 0
                timed(calls["route"])
                assert routed.counts() == [n, 0, 0, 0, 0, 0, 0, 0]
                timed(calls["key_phase"])
                if a.only:
                    for _ in range(a.reps):
                        timed(calls[a.only])
                    continue
                T = {k: [] for k in CALLS}
                for _ in range(a.reps):
                    for k in CALLS:
                        T[k].append(timed(calls[k]))
                res[f"{form}_{n}"] = {k: spread(v) for k, v in T.items()}
                del wire, r_out
            del plain
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
