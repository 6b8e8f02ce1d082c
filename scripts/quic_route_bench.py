#!/usr/bin/env python3
"""Measures the datagram router against the open it feeds.

One process; per batch size and wire form (plain, under Salamander) the
routes alternate within each repetition; median and min-max:
  route      sqobfs_quic_route(_salamander) alone
  key_phase  sqobfs_quic_key_phase(_salamander) alone: the nearest existing
             kernel (same bytes read, same BLAKE2b key under Salamander)
  chained    route, the host reads count[8], key_phase and open on the SHORT
             slice
  prepared   key_phase + open with key_id, pn_offset and pn prepared on the
             host beforehand (not timed): what a caller did before the router
The batch: N short-header datagrams of 1,350 bytes (+ 8 under Salamander)
over 1,024 connections with 8-byte connection ids, AES-128-GCM, both key
phases.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sing-quic_amd"))
import sqobfs  # noqa: E402

DGRAM, SLOT, CONNS, PNO = 1350, 1376, 1024, 9


def spread(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 1), "min_us": round(min(xs) * 1e6, 1),
            "max_us": round(max(xs) * 1e6, 1), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65535, 1 << 20])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=["route"], default=None,
                    help="that route alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the CPU"
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(944))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    cids = rng.integers(0, 256, (CONNS, 8), dtype=np.uint8)
    cids[:, :2] = np.arange(CONNS, dtype=">u2").view(np.uint8).reshape(CONNS, 2)  # distinct
    res = {"datagram_bytes": DGRAM, "conns": CONNS}
    with sqobfs.Context(0) as ctx, \
            sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [b"sing-quic-mi355x-bench-psk"]) as okr, \
            sqobfs.QuicKeyring.from_secrets(
                ctx, [sqobfs.QuicSecret.of(rng.bytes(32)) for _ in range(CONNS)],
                sqobfs.QUIC_AES_128_GCM) as kr, \
            sqobfs.QuicCidMap(ctx, CONNS, 2 * CONNS, 8) as cmap:
        cmap.update([(bytes(c), i) for i, c in enumerate(cids)])

        def timed(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        for n in a.n:
            conn = rng.integers(0, CONNS, n)
            phase = rng.integers(0, 2, n)
            pns = np.arange(n, dtype=np.uint64)
            plain = torch.randint(0, 256, (n, SLOT), dtype=torch.uint8, device=dev)
            plain[:, 0] = t((0x43 | (phase << 2)).astype(np.uint8))
            plain[:, 1:9] = t(cids[conn])
            plain[:, 9:13] = t(pns.astype(">u4").view(np.uint8).reshape(n, 4))
            off = t(np.arange(n, dtype=np.uint64) * SLOT)
            len_p = t(np.full(n, DGRAM - 16, np.uint32))
            out_len, pn_out = t(np.zeros(n, np.uint32)), t(np.zeros(n, np.uint64))
            ids, zero = t(np.zeros(n, np.uint16)), t(np.zeros(n, np.uint64))
            pno, kid0 = t(np.full(n, PNO, np.uint16)), t((2 * conn).astype(np.uint16))
            d_back = torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
            want = plain[:, :DGRAM - 16]
            for form in ("plain", "salamander"):
                ob = form == "salamander"
                wire = torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
                len_w = t(np.full(n, DGRAM + 8 * ob, np.uint32))
                bs = sqobfs.quic_batch(n, plain.view(-1), off, len_p, wire, off, out_len, pno,
                                       t(pns), t((2 * conn + phase).astype(np.uint16)))
                if ob:
                    sqobfs.quic_seal_salamander(ctx, kr, okr, bs,
                                                t(rng.integers(0, 256, n * 8, dtype=np.uint8)))
                else:
                    sqobfs.quic_seal(ctx, kr, bs)
                ctx.sync()
                routed = sqobfs.QuicRouted(n, dev)
                b_in = sqobfs.quic_batch(n, wire, off, len_w, None, off, None, None, None)
                b_res = sqobfs.quic_batch(n, wire, off, len_w, d_back, off, out_len, pno, zero, kid0)
                b_open = sqobfs.quic_batch(n, wire, off, len_w, d_back, off, out_len, pno, zero, ids,
                                           pn_out)
                if ob:
                    route = lambda: sqobfs.quic_route_salamander(ctx, cmap, okr, b_in, routed)  # noqa: E731
                    resolve = lambda b: sqobfs.quic_key_phase_salamander(ctx, kr, okr, b, ids)  # noqa: E731
                    opn = lambda b: sqobfs.quic_open_salamander(ctx, kr, okr, b)  # noqa: E731
                else:
                    route = lambda: sqobfs.quic_route(ctx, cmap, b_in, routed)  # noqa: E731
                    resolve = lambda b: sqobfs.quic_key_phase(ctx, kr, b, ids)  # noqa: E731
                    opn = lambda b: sqobfs.quic_open(ctx, kr, b)  # noqa: E731

                def chained():
                    route()
                    counts = routed.counts()  # the host's only read: 32 bytes
                    b = routed.batch(sqobfs.QUIC_ROUTE_SHORT, counts, wire, d_back, out_len, pn_out)
                    resolve(b)
                    b.key_id = ids.data_ptr()
                    opn(b)
                    return counts

                def prepared():
                    resolve(b_res)
                    opn(b_open)

                for fn in (chained, prepared):  # warm-up, and the routes agree
                    d_back.zero_()
                    timed(fn)
                    assert bool((out_len == DGRAM - 16).all()) and bool((pn_out == t(pns)).all())
                    assert torch.equal(d_back.view(n, SLOT)[:, :DGRAM - 16], want)
                assert routed.counts() == [n, 0, 0, 0, 0, 0, 0, 0]
                assert np.array_equal(routed.key_id.cpu().numpy(), 2 * conn)
                assert np.array_equal(routed.conn.cpu().numpy(), conn)
                if a.only == "route":
                    for _ in range(a.reps):
                        timed(route)
                    continue
                T = {"route": [], "key_phase": [], "chained": [], "prepared": []}
                for _ in range(a.reps):
                    T["route"].append(timed(route))
                    T["key_phase"].append(timed(lambda: resolve(b_res)))
                    T["chained"].append(timed(chained))
                    T["prepared"].append(timed(prepared))
                res[f"{form}_{n}"] = {k: spread(v) for k, v in T.items()}
                del wire
            del plain, d_back
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
