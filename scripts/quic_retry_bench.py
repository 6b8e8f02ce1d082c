#!/usr/bin/env python3
"""Measures Retry building and token validation against the
Initial open that a listener pays per unvalidated Initial without them.

One process; per batch size and wire form (plain, under Salamander) the calls
alternate within each repetition; median and min-max:
  retry         sqobfs_quic_retry(_salamander), library tokens
  retry_check   sqobfs_quic_retry_check(_salamander)
  initial_open  sqobfs_quic_initial_open(_salamander) on the same batch
The batch: N sealed client Initials of 1,200 bytes (+ 8 under Salamander) with
8-byte connection ids, each carrying the 53-byte token of the Retry that
answered its first flight.  Before timing, a sample of the Retries is compared
with the Python reference over the CPU oracle's AES-GCM, and every token must
check OK with its ODCID.  Prints one JSON line and writes it to --out.
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import sqobfs  # noqa: E402

DGRAM, SLOT, CID, SAMPLE = 1200, 1216, 8, 512
PSK = b"sing-quic-mi355x-bench-psk"
TKEY, TIV = bytes(range(16)), bytes(range(12))
RKEY, RNONCE = bytes.fromhex("be0c690b9f66575a1d766b54e368c84e"), bytes.fromhex("461599d35d632bf2239825bb")


def spread(xs):
    return {"median_us": round(statistics.median(xs) * 1e6, 1), "min_us": round(min(xs) * 1e6, 1),
            "max_us": round(max(xs) * 1e6, 1), "reps": len(xs)}


def ref_retry(ol, odcid, scid, rscid, nonce, addr, now):
    iv = bytes(a ^ b for a, b in zip(TIV, nonce))
    tok = nonce + ol.gcm_seal(TKEY, iv, addr + bytes([CID]) + rscid.ljust(20, b"\0"),
                              now.to_bytes(4, "big") + bytes([CID]) + odcid.ljust(20, b"\0"))
    body = b"\xf0\x00\x00\x00\x01" + bytes([CID]) + scid + bytes([CID]) + rscid + tok
    return body + ol.gcm_seal(RKEY, RNONCE, bytes([CID]) + odcid + body, b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65535, 1 << 20])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=["retry", "retry_check", "initial_open"], default=None,
                    help="that call alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import oracle_lib as ol
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on the CPU"
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(945))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)  # noqa: E731
    now, res = 1_800_000_000, {"datagram_bytes": DGRAM, "cid_bytes": CID}
    with sqobfs.Context(0) as ctx, sqobfs.Keyring(ctx, sqobfs.SALAMANDER, [PSK]) as okr, \
            sqobfs.QuicKeyring(ctx, [sqobfs.QuicKey.of(TKEY, TIV, bytes(16))],
                               sqobfs.QUIC_AES_128_GCM) as tkr:

        def timed(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        for n in a.n:
            off = t(np.arange(n, dtype=np.uint64) * SLOT)
            out_len, pn = t(np.zeros(n, np.uint32)), t(np.zeros(n, np.uint64))
            dcid, scid, rscid = rnd(n, CID), rnd(n, CID), rnd(n, 20)
            addr, nonce, salt = rnd(n, 18), rnd(n, 12), rnd(n, 8)
            r_out, r_off = torch.zeros(n * 144, dtype=torch.uint8, device=dev), \
                t(np.arange(n, dtype=np.uint64) * 144)
            args = sqobfs.quic_retry_args(tkr, addr.view(-1), nonce.view(-1), rscid.view(-1), CID, now)

            def flight(ob, dc, token):
                """Sealed client Initials of DGRAM bytes with DCID dc: (wire, in_len)."""
                tl = 0 if token is None else 53
                pno = 1 + 4 + 1 + CID + 1 + CID + 1 + tl + 2
                u = rnd(n, SLOT)
                u[:, 0] = 0xC1
                u[:, 1:6] = t(np.array([0, 0, 0, 1, CID], np.uint8))
                u[:, 6:6 + CID] = dc
                u[:, 6 + CID] = CID
                u[:, 7 + CID:7 + 2 * CID] = scid
                u[:, 7 + 2 * CID] = tl
                if tl:
                    u[:, 8 + 2 * CID:pno - 2] = token
                u[:, pno - 2:pno] = t(np.frombuffer((0x4000 | (DGRAM - pno)).to_bytes(2, "big"), np.uint8))
                u[:, pno:pno + 2] = 0  # packet number 0
                wire = torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
                b = sqobfs.quic_batch(n, u.view(-1), off, t(np.full(n, DGRAM - 16, np.uint32)), wire,
                                      off, out_len, None, pn)
                if ob:
                    sqobfs.quic_initial_seal_salamander(ctx, okr, b, sqobfs.QUIC_SIDE_CLIENT,
                                                        salt=rnd(n * 8))
                else:
                    sqobfs.quic_initial_seal(ctx, b, sqobfs.QUIC_SIDE_CLIENT)
                ctx.sync()
                assert bool((out_len == DGRAM + 8 * ob).all())
                return wire, t(np.full(n, DGRAM + 8 * ob, np.uint32))

            def retry_of(ob, wire, len_w):
                b = sqobfs.quic_batch(n, wire, off, len_w, r_out, r_off, out_len, None, None)
                return lambda: sqobfs.quic_retry(ctx, b, args, okr if ob else None, salt.view(-1))

            # the first flight's Retries (plain form) give the tokens of both forms
            rlen = 7 + 2 * CID + 53 + 16
            timed(retry_of(False, *flight(False, dcid, None)))
            assert bool((out_len == rlen).all())
            token = r_out.view(n, 144)[:, 7 + 2 * CID:rlen - 16].clone()
            h = {k: v[:SAMPLE].cpu().numpy() for k, v in dict(d=dcid, s=scid, r=rscid, a=addr,
                                                              nn=nonce, sa=salt).items()}
            want = [ref_retry(ol, h["d"][i].tobytes(), h["s"][i].tobytes(), h["r"][i, :CID].tobytes(),
                              h["nn"][i].tobytes(), h["a"][i].tobytes(), now)
                    for i in range(min(n, SAMPLE))]
            for form in ("plain", "salamander"):
                ob = form == "salamander"
                wire, len_w = flight(ob, rscid[:, :CID], token)  # the client's answer to the Retry
                run_retry = retry_of(ob, wire, len_w)
                timed(run_retry)  # (its ODCID is the rscid of the first: a listener would not, the cost is the same)
                got = r_out.view(n, 144)[:SAMPLE].cpu().numpy()
                for i, w in enumerate(want):
                    w = ref_retry(ol, h["r"][i, :CID].tobytes(), h["s"][i].tobytes(),
                                  h["r"][i, :CID].tobytes(), h["nn"][i].tobytes(), h["a"][i].tobytes(), now)
                    w = ol.salamander_write(PSK, h["sa"][i].tobytes(), w)[0] if ob else w
                    assert got[i, :len(w)].tobytes() == w, (form, i)
                assert token[:SAMPLE].cpu().numpy().tobytes() == b"".join(x[7 + 2 * CID:-16] for x in want)
                st, od = t(np.zeros(n, np.uint8)), torch.zeros(n * 20, dtype=torch.uint8, device=dev)
                odl, o_out = t(np.zeros(n, np.uint8)), torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
                b_in = sqobfs.quic_batch(n, wire, off, len_w, None, None, None, None, None)
                b_open = sqobfs.quic_batch(n, wire, off, len_w, o_out, off, out_len, None, pn)
                cargs = sqobfs.quic_retry_args(tkr, addr.view(-1), now=now + 5, max_age=10)
                run_check = lambda: sqobfs.quic_retry_check(ctx, b_in, cargs, st, od, odl, None,  # noqa: E731
                                                            okr if ob else None)
                if ob:
                    run_open = lambda: sqobfs.quic_initial_open_salamander(  # noqa: E731
                        ctx, okr, b_open, sqobfs.QUIC_SIDE_CLIENT)
                else:
                    run_open = lambda: sqobfs.quic_initial_open(ctx, b_open, sqobfs.QUIC_SIDE_CLIENT)  # noqa: E731
                timed(run_check)
                assert bool((st == sqobfs.QUIC_TOKEN_OK).all()) and bool((odl == CID).all())
                assert torch.equal(od.view(n, 20)[:, :CID], dcid)
                timed(run_open)
                assert bool((out_len == DGRAM - 16).all())
                calls = {"retry": run_retry, "retry_check": run_check, "initial_open": run_open}
                if a.only:
                    for _ in range(a.reps):
                        timed(calls[a.only])
                    continue
                T = {k: [] for k in calls}
                for _ in range(a.reps):
                    for k, fn in calls.items():
                        T[k].append(timed(fn))
                res[f"{form}_{n}"] = {k: spread(v) for k, v in T.items()}
                del wire, o_out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
