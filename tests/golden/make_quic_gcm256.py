"""Generate tests/golden/quic_gcm256.json: QUIC packets protected with
TLS_AES_256_GCM_SHA384 (AES-256-GCM payload protection, AES-256 header
protection; RFC 9001 5.3 / 5.4.3), built with OpenSSL (ctypes on libcrypto).
Run from the repo root:  python tests/golden/make_quic_gcm256.py

OpenSSL is first pinned to FIPS-197 C.3 and to test cases 13 and 14 of the GCM
specification.  Deterministic: numpy PCG64 with fixed seeds."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np

from make_quic_gcm import _L, B  # libcrypto with its argument types declared

_L.EVP_aes_256_gcm.restype = _L.EVP_aes_256_ecb.restype = ctypes.c_void_p


def evp(cipher, key: bytes, iv, aad: bytes, pt: bytes) -> bytes:
    """ECB (iv None: one block) or GCM (ciphertext || tag) of pt."""
    c, n = _L.EVP_CIPHER_CTX_new(), ctypes.c_int(0)
    assert _L.EVP_EncryptInit_ex(c, cipher, None, key, iv) == 1
    _L.EVP_CIPHER_CTX_set_padding(c, 0)
    if aad:
        assert _L.EVP_EncryptUpdate(c, None, ctypes.byref(n), aad, len(aad)) == 1
    out, tag = ctypes.create_string_buffer(len(pt) + 16), ctypes.create_string_buffer(16)
    if pt:
        assert _L.EVP_EncryptUpdate(c, out, ctypes.byref(n), pt, len(pt)) == 1
    assert _L.EVP_EncryptFinal_ex(c, out, ctypes.byref(n)) == 1
    if iv is not None:
        assert _L.EVP_CIPHER_CTX_ctrl(c, 0x10, 16, tag) == 1  # EVP_CTRL_AEAD_GET_TAG
    _L.EVP_CIPHER_CTX_free(c)
    return out.raw[:len(pt)] + (tag.raw if iv is not None else b"")


def quic_seal(key, iv, hp, pn, pkt, pn_offset):
    pn_len = (pkt[0] & 3) + 1
    hdr = pn_offset + pn_len
    nonce = bytes(a ^ b for a, b in zip(iv, pn.to_bytes(12, "big")))
    out = bytearray(pkt[:hdr] + evp(_L.EVP_aes_256_gcm(), key, nonce, pkt[:hdr], pkt[hdr:]))
    mask = evp(_L.EVP_aes_256_ecb(), hp, None, b"", bytes(out[pn_offset + 4:pn_offset + 20]))
    out[0] ^= mask[0] & (0x0F if out[0] & 0x80 else 0x1F)
    for i in range(pn_len):
        out[pn_offset + i] ^= mask[1 + i]
    return bytes(out)


def main() -> None:
    z = bytes(32)
    assert evp(_L.EVP_aes_256_ecb(), bytes(range(32)), None, b"",
               B("00112233445566778899aabbccddeeff")).hex() == "8ea2b7ca516745bfeafc49904b496089"
    assert evp(_L.EVP_aes_256_gcm(), z, z[:12], b"", b"").hex() == \
        "530f8afbc74536b9a963b4f1c4cb738b"
    assert evp(_L.EVP_aes_256_gcm(), z, z[:12], b"", z[:16]).hex() == \
        "cea7403d4d606b6e074ec5d3baf39d18" "d0d1c8a799996bf0265b98b5d48ab919"
    rng = np.random.Generator(np.random.PCG64(9256))
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731

    def record(key, iv, hp, i, plen, long_hdr):
        pn_len = max(1 + i % 4, 4 - plen)
        dcid = int(rng.integers(0, 21))
        first = (0xC0 if long_hdr else 0x40) | int(rng.integers(0, 16)) << 2 & 0x3C | (pn_len - 1)
        pn_offset = 1 + dcid + (6 if long_hdr else 0)
        pn = int(rng.integers(0, 2**62)) if i % 3 else int(rng.integers(0, 2**16))
        pkt = bytes([first]) + rb(pn_offset - 1) + \
            (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big") + rb(plen)
        return {"pn": pn, "largest_pn": max(0, pn - int(rng.integers(1, 2 ** (8 * pn_len - 2)))),
                "pn_offset": pn_offset, "packet": pkt.hex(),
                "protected": quic_seal(key, iv, hp, pn, pkt, pn_offset).hex()}
    packets = []
    for i in range(40):
        key, iv, hp = rb(32), rb(12), rb(32)
        plen = int(rng.integers(0, 301)) if i % 7 else 0
        packets.append({"key": key.hex(), "iv": iv.hex(), "hp": hp.hex(),
                        **record(key, iv, hp, i, max(plen, 3 - i % 4), i % 5 == 4)})
    keys = [(rb(32), rb(12), rb(32)) for _ in range(2)]
    edge = [1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 2064, 4000]
    stream = []
    for k in range(2):
        for i in range(32):
            plen = edge[i] if k == 0 and i < len(edge) else int(rng.integers(3, 301))
            stream.append({"k": k, **record(*keys[k], i, plen, False)})
    out = {"_doc": "QUIC AES-256-GCM packet protection vectors built with OpenSSL; see "
                   "make_quic_gcm256.py",
           "packets": packets, "stream": stream,
           "stream_keys": [{"key": a.hex(), "iv": b.hex(), "hp": c.hex()} for a, b, c in keys]}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "quic_gcm256.json"),
              "w") as f:
        json.dump(out, f, indent=1)
    print("wrote quic_gcm256.json:", len(packets), "packets,", len(stream), "stream records")


if __name__ == "__main__":
    main()
