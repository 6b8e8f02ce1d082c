// sq_quic_initial.hip -- gfx950 QUIC v1 Initial packet protection with the
// keys derived per packet on the device (RFC 9001 5.2-5.4, AEAD_AES_128_GCM;
// long header: RFC 9000 17.2.2).
//
// Replaces, for a whole ragged batch per launch, what quic-go does per packet
// and per new connection on the host
//   internal/handshake/initial_aead.go  NewInitialAEAD / computeSecrets
//   internal/handshake/aead.go, header_protector.go, internal/wire/header.go
// (quic-go v0.52.0-beta.1, go.mod:7; reached from the reference through
// quic.go:47-102; not in the reference tree).  Initial keys come from the
// client's first Destination Connection ID, so a listening port meets a new
// key with every new client and every probe: there is no keyring here, and
// no per-key table that a later packet could reuse.  Hysteria2 wire
// datagrams (salt8 || packet ^ BLAKE2b-256(psk || salt8)) take the OB
// instantiations of both kernels (sqobfs_quic_initial_open_salamander /
// _seal_salamander): the Salamander layer comes off, or goes on, in the same
// pass, with no launch and no buffer in between.
//
// Work decomposition, two kernels per call:
//   1. quic_initial_keys: one lane per packet, 64 packets per wave.  The
//      lane parses the long header (first 32 bytes in registers, longer
//      tokens byte by byte), runs HKDF-Extract(salt, dcid) from the salt's
//      pad midstates (launch constants), Expand-Label "client in" /
//      "server in", then key, iv and hp from that secret's shared pad
//      midstates: 14 SHA-256 compressions.  It expands the AES-128 packet
//      key, computes H = E(K, 0) and H^2..H^4 by the bitwise multiply, and
//      writes a 288-byte record (QInitRec).  A packet that fails a header
//      check gets its error code and no keys.
//   2. quic_initial_protect: four lanes (a quad) per packet, 16 packets per
//      wave.  The wave stages its packets' round keys in LDS; each quad
//      builds one 4-bit Shoup table of H^4 (256 B).  GHASH runs over the
//      padded AAD blocks, the ciphertext blocks and the lengths block as one
//      sequence of N blocks: quad lane j takes blocks j, j + 4, ... with
//      Y = (Y ^ X) * H^4 through the table, leaves its last block
//      unmultiplied, multiplies once by the H^1..H^4 (bitwise) that this
//      block's distance from the end calls for, and the quad XOR-reduces by
//      DPP.  AES-CTR follows the same interleave (the payload block of GHASH
//      block b is encrypted by the lane that hashes it), so a quad's loads
//      and stores of one step cover 64 contiguous bytes.  Header protection
//      is one AES block under the hp key, expanded round by round in
//      registers; the four lanes compute it redundantly (the same wave
//      instructions as one lane would take, and no broadcast).
//
// The fused Salamander layer (template flag OB; the OB = false code is what it
// was).  Key byte k covers packet byte k mod 32, so the period is aligned to
// packet byte 0 and every offset below is the packet's, not the datagram's.
//   keys<OB>:    the lane derives K from the keyring's PSK state (entry 0) and
//      the packet's salt (open: the first 8 wire bytes; seal: salt[i])
//      before HKDF, whose registers it then reuses; open XORs the 32 head
//      bytes in registers (hd ^= K) and each varint byte past byte 32 with
//      K[p & 31] as it is loaded.  K goes to the packet kernel through the
//      workspace, in a 32-byte slot after the n records.
//   protect<.., OB>: each lane holds K, and K rotated to the payload start
//      (hdr & 31): payload block c takes half c & 1 of the rotated key,
//      16-aligned header block b takes half b & 1 of K.  Open XORs on load
//      (header blocks past byte 32, payload blocks, sample, tag) and then
//      copies the datagram's remainder (coalesced packets), 64 bytes per quad
//      step, de-obfuscated with K rotated to span & 31.  Seal hashes and
//      samples the plain ciphertext and XORs only what it stores, the tag and
//      the protected first byte and packet-number bytes included; quad lane 0
//      writes the salt.  In place, open's output lies 8 bytes below its
//      input: see the comments at the loads.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "sq_bytes.h"
#include "sq_hash.h"
#include "sq_internal.h"
#include "sq_obfs_key.h"
#include "sq_quic.h"
#include "sq_quic_aes.h"
#include "sq_quic_kdf.h"

namespace sq {

constexpr uint32_t kIKBlock = 64;   // keys: one wave per workgroup (spreads small batches)
constexpr uint32_t kIBlock = 768;   // protect: 12 waves, one workgroup per CU
constexpr uint32_t kIWaves = kIBlock / kWave;
constexpr uint32_t kIPpw = kWave / 4;  // packets per wave: one per quad

// ---------------------------------------------------------------- keys

// HMAC over one message block that follows the inner pad (msg: padded, with
// the length), from the key's pad midstates
__device__ __forceinline__ void hmac_block(const uint32_t (&im)[8], const uint32_t (&om)[8],
                                           const uint32_t (&msg)[16], uint32_t (&out)[12]) {
  uint32_t st[8], m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = im[i];
  s2_compress(st, msg);
#pragma unroll
  for (int i = 0; i < 8; i++) m[i] = st[i];
  m[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) m[i] = 0u;
  m[15] = (64u + 32u) * 8u;
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = om[i];
  s2_compress(st, m);
#pragma unroll
  for (int i = 0; i < 12; i++) out[i] = i < 8 ? st[i & 7] : 0u;
}

// byte offset of packet i's Salamander key in the workspace of n packets
__device__ __forceinline__ uint64_t okey_slot(const QInitParams &P, uint32_t i) {
  return (uint64_t)(P.rec + P.n) + 32ull * i;
}

template <bool OB>
__global__ __launch_bounds__(kIKBlock) void quic_initial_keys(const QInitParams P) {
  __shared__ uint32_t T[256];
  stage_t0<kIKBlock>(P.t0, T);
  const uint32_t i = blockIdx.x * kIKBlock + threadIdx.x;
  if (i >= P.n) return;
  uint64_t src = (uint64_t)P.in + P.in_off[i];
  uint32_t len = P.in_len[i];
  const uint64_t rec = (uint64_t)(P.rec + i);
  uint32_t hd[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, pno = 0, span = 0;
  uint32_t okey[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  uint64_t length = 0;
  if (OB) {  // the packet's Salamander key, before HKDF needs the registers
    uint32_t osalt[4] = {0u, 0u, 0u, 0u};
    if (!P.open) {
      const u32x2 sv = gld<u32x2>((uint64_t)P.salt + 8ull * i);
      osalt[0] = sv.x;
      osalt[1] = sv.y;
    } else if (len >= (uint32_t)kSalamanderSalt && len <= kQMaxPacket) {
      load16(src, src + kSalamanderSalt, osalt);  // the first 8 wire bytes (salamander.go:50)
      src += kSalamanderSalt;
      len -= kSalamanderSalt;
    } else {
      len = 0;  // too short for a salt: rejected below
    }
    if (len) {
      salamander_key(P.opsk, osalt, okey);
      const uint64_t slot = okey_slot(P, i);
      gst<u32x4>(slot, u32x4{okey[0], okey[1], okey[2], okey[3]});
      gst<u32x4>(slot + 16, u32x4{okey[4], okey[5], okey[6], okey[7]});
    }
  }
  uint32_t err = len == 0 || len > kQMaxPacket ? kQEShort : 0u;
  if (!err) {
    load_head32(src, len, hd);
    if (OB) {  // open: the key period starts at packet byte 0; seal parses plain input
      const uint32_t om = P.open ? 0xFFFFFFFFu : 0u;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        okey[j] &= om;
        hd[j] ^= okey[j] & range_mask(0, (int)(len < 32 ? len : 32), j);
      }
    }
    err = parse_initial<OB>(hd, src, len, P.version, pno, length, okey);
  }
  if (!err) {
    if (P.open) {  // the packet is [0, pno + Length): coalesced packets may follow
      if (length > len - pno || pno + 4 + 16 > pno + (uint32_t)length) err = kQEShort;
      span = pno + (uint32_t)length;
    } else {  // in = header || payload, all of len: Length = pn_len + payload + 16
      if (pno + length != (uint64_t)len + 16) err = kQEHeader;
      else if (pno + 4 > len) err = kQEShort;  // (as sqobfs_quic_seal: room to sample)
      span = len;
    }
  }
  // the connection's original DCID: given, or the packet's own (bytes 6 ..)
  uint32_t d[5], dl = (hd[1] >> 8) & 0xFFu;
#pragma unroll
  for (int j = 0; j < 5; j++) d[j] = __builtin_amdgcn_alignbyte(hd[j + 2], hd[j + 1], 2);
  if (P.odcid) {
    dl = P.odcid_len[i];
    if (dl > kMaxCid) {
      if (!err) err = kQEHeader;
    } else {
#pragma unroll
      for (int j = 0; j < 5; j++) d[j] = gld<uint32_t>((uint64_t)P.odcid + 20ull * i + 4 * j);
    }
  }
  if (err) {
    gst<uint32_t>(rec + offsetof(QInitRec, err), err);
    return;
  }
  // initial_secret = HKDF-Extract(salt, dcid) = HMAC(salt, dcid): one block
  uint32_t m[16], o[12];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    uint32_t w = (j < 5 ? d[j] : 0u) & range_mask(0, (int)dl, j);
    w |= bsel((dl >> 2) == (uint32_t)j, 0x80u << (8 * (dl & 3)), 0u);
    m[j] = __builtin_bswap32(w);
  }
#pragma unroll
  for (int j = 6; j < 15; j++) m[j] = 0u;
  m[15] = (64u + dl) * 8u;
  hmac_block(P.salt_im, P.salt_om, m, o);
  Prf<false> prf;
  prf.set_key(o);
  hmac_block(prf.im, prf.om, P.side_msg, o);  // client / server initial secret
  prf.set_key(o);
  uint32_t key[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, rk[44];
  hmac_block(prf.im, prf.om, P.key_msg, o);
#pragma unroll
  for (int j = 0; j < 4; j++) key[j] = __builtin_bswap32(o[j]);
  aes_expand<4>(T, key, rk);
  store_schedule<4>(rec, rk);
  hmac_block(prf.im, prf.om, P.iv_msg, o);
  gst<u32x4>(rec + offsetof(QInitRec, iv),
             u32x4{__builtin_bswap32(o[0]), __builtin_bswap32(o[1]), __builtin_bswap32(o[2]), 0u});
  hmac_block(prf.im, prf.om, P.hp_msg, o);
  gst<u32x4>(rec + offsetof(QInitRec, hp),
             u32x4{__builtin_bswap32(o[0]), __builtin_bswap32(o[1]), __builtin_bswap32(o[2]),
                   __builtin_bswap32(o[3])});
  uint32_t h[4] = {0u, 0u, 0u, 0u};  // H = E(K, 0^128)
  aes_block_t0<10, false>(T, [&](int r, uint32_t (&k)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) k[c] = rk[4 * r + c];
  }, h);
  const G4 h1 = {{__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]),
                  __builtin_bswap32(h[3])}};
  const G4 h2 = g_mul(h1, h1), h3 = g_mul(h2, h1), h4 = g_mul(h2, h2);
  const G4 hs[4] = {h1, h2, h3, h4};
#pragma unroll
  for (int k = 0; k < 4; k++)
    gst<u32x4>(rec + offsetof(QInitRec, h) + 16 * k,
               u32x4{hs[k].w[0], hs[k].w[1], hs[k].w[2], hs[k].w[3]});
  gst<u32x4>(rec + offsetof(QInitRec, pn_offset), u32x4{pno, span, 0u, 0u});
}
static_assert(offsetof(QInitRec, rk) == 0 && offsetof(QInitRec, iv) % 16 == 0 &&
                  offsetof(QInitRec, err) == offsetof(QInitRec, iv) + 12 &&
                  offsetof(QInitRec, hp) % 16 == 0 && offsetof(QInitRec, h) % 16 == 0 &&
                  offsetof(QInitRec, pn_offset) % 16 == 0 &&
                  offsetof(QInitRec, span) == offsetof(QInitRec, pn_offset) + 4,
              "16-byte vector accesses to the record");

// ---------------------------------------------------------------- protect

// A wave's LDS: its 16 packets' round keys (a quad's reads broadcast), their
// Shoup tables of H^4 (entry n in slot n ^ packet slot, so quads in the same
// state read different slots) and, seal, ciphertext bytes 0..31 (the
// header-protection sample).
struct alignas(16) IWave {
  uint32_t rk[kIPpw][44];
  uint32_t tab[kIPpw][64];
  uint32_t ct32[kIPpw][8];
};
constexpr uint32_t kILdsWords = 256 * 64 + kIWaves * (uint32_t)sizeof(IWave) / 4;
// 64 KiB of T-tables and 7,424 B per wave: 154,624 B with 12 waves
static_assert(kILdsWords * 4 <= 160 * 1024, "the LDS image exceeds gfx950's 160 KiB per workgroup");

// 5 header-protection mask bytes (RFC 9001 5.4.3): AES-128-ECB(hp, sample)
// with the key expanded on the fly, one round key ahead of the round that
// uses it (FIPS-197 5.2; S-box = byte 1 of T0, as sq_quic_kdf.h sub_word)
__device__ __forceinline__ void hp_mask_otf(const uint32_t *tT, uint32_t lo,
                                            const uint32_t (&hp)[4], const uint32_t (&sample)[4],
                                            uint32_t &m0, uint32_t &m1) {
  uint32_t k[4], s[4], t[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    k[c] = hp[c];
    s[c] = sample[c] ^ k[c];
  }
#pragma unroll
  for (int r = 1; r <= 10; r++) {
    const uint32_t rw = rotl(k[3], 24);  // RotWord
    const uint32_t b0 = t0at(tT, trow(rw, lo, 0)), b1 = t0at(tT, trow(rw, lo, 1));
    const uint32_t b2 = t1at(tT, trow(rw, lo, 2)), b3 = t1at(tT, trow(rw, lo, 3));
    k[0] ^= __builtin_amdgcn_perm(b1, b0, 0x0C0C0501u) ^
            __builtin_amdgcn_perm(b3, b2, 0x07020C0Cu) ^ aes_rcon(r - 1);
    k[1] ^= k[0];
    k[2] ^= k[1];
    k[3] ^= k[2];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t a0 = t0at(tT, trow(s[c], lo, 0));
      if (r < 10) {
        const uint32_t a1 = t1at(tT, trow(s[(c + 1) & 3], lo, 1));
        const uint32_t a2 = t0at(tT, trow(s[(c + 2) & 3], lo, 2));
        const uint32_t a3 = t1at(tT, trow(s[(c + 3) & 3], lo, 3));
        t[c] = xor3(a0, a1, rotl(a2 ^ a3, 16)) ^ k[c];
      } else {  // (the last round's byte picks, as aes_encrypt_n)
        const uint32_t a1 = t0at(tT, trow(s[(c + 1) & 3], lo, 1));
        const uint32_t a2 = t1at(tT, trow(s[(c + 2) & 3], lo, 2));
        const uint32_t a3 = t1at(tT, trow(s[(c + 3) & 3], lo, 3));
        t[c] = xor3(__builtin_amdgcn_perm(a1, a0, 0x0C0C0501u),
                    __builtin_amdgcn_perm(a3, a2, 0x07020C0Cu), k[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = t[c];
  }
  m0 = s[0];
  m1 = s[1] & 0xFFu;
}

// XOR over the four lanes of a quad (DPP quad_perm [1,0,3,2], then [2,3,0,1])
__device__ __forceinline__ uint32_t quad_xor(uint32_t v) {
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  return v;
}

// w ^= half `odd` of the 32-byte key k (bytes 16 odd .. 16 odd + 15)
__device__ __forceinline__ void xor_half(uint32_t (&w)[4], const uint32_t (&k)[8], bool odd) {
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] ^= bsel(odd, k[4 + i], k[i]);
}

// the 32-byte key k rotated left by r bytes: out byte i = k[(r + i) & 31]
__device__ __forceinline__ void key_rot(const uint32_t (&k)[8], uint32_t r, uint32_t (&out)[8]) {
  uint32_t a[4], b[4];
  keywin(k, r, a);
  keywin(k, r + 16, b);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[i] = a[i];
    out[4 + i] = b[i];
  }
}

// One unit of a wave: packets [base, base + 16), packet slot q = lane / 4.
template <bool OPEN, bool OB>
__device__ __forceinline__ void initial_unit(const QInitParams &P, uint64_t base, uint32_t lane,
                                             const uint32_t *tT, uint32_t tcol, IWave &W) {
  const uint32_t q = lane >> 2, j = lane & 3;
  // the unit's round keys: 16 x 11 vectors of 16 bytes, 64 lanes
  for (uint32_t v = lane; v < kIPpw * 11; v += kWave) {
    const uint32_t pk = v / 11, r = v - 11 * pk;
    if (base + pk < P.n)
      *(u32x4 *)&W.rk[pk][4 * r] = gld<u32x4>((uint64_t)(P.rec + base + pk) + 16ull * r);
  }
  if (base + q >= P.n) return;
  const uint32_t p = (uint32_t)(base + q);
  const uint64_t rec = (uint64_t)(P.rec + p);
  const u32x4 ive = gld<u32x4>(rec + offsetof(QInitRec, iv));
  if (ive.w) {  // rejected by the key kernel
    if (j == 0) {
      P.out_len[p] = ive.w;
      if (OPEN && P.pn_out) P.pn_out[p] = 0;
    }
    return;
  }
  const u32x4 hpv = gld<u32x4>(rec + offsetof(QInitRec, hp));
  const u32x4 h4v = gld<u32x4>(rec + offsetof(QInitRec, h) + 48);
  const u32x4 meta = gld<u32x4>(rec + offsetof(QInitRec, pn_offset));
  const uint32_t pno = meta.x, len = meta.y;  // len: the packet's bytes (open: its span)
  // OB: the packet follows the 8 salt bytes of the wire datagram (open: in,
  // seal: out); src, dst and every offset below are the packet's
  const uint64_t wire = OPEN ? (uint64_t)P.in + P.in_off[p] : (uint64_t)P.out + P.out_off[p];
  const uint64_t src = OB && OPEN ? wire + kSalamanderSalt : (uint64_t)P.in + P.in_off[p];
  const uint64_t dst = OB && !OPEN ? wire + kSalamanderSalt : (uint64_t)P.out + P.out_off[p];
  const uint32_t hp[4] = {hpv.x, hpv.y, hpv.z, hpv.w}, iv[3] = {ive.x, ive.y, ive.z};
  uint32_t ok[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the packet's Salamander key
  if (OB) {
    const u32x4 a = gld<u32x4>(okey_slot(P, p)), b = gld<u32x4>(okey_slot(P, p) + 16);
    ok[0] = a.x; ok[1] = a.y; ok[2] = a.z; ok[3] = a.w;
    ok[4] = b.x; ok[5] = b.y; ok[6] = b.z; ok[7] = b.w;
  }
  // packet byte k as it is read (open: de-obfuscated)
  auto hb = [&](const uint32_t (&h)[8], uint32_t k) -> uint32_t {
    const uint32_t v = head_byte(h, src, k);
    return (OB && OPEN && k >= 32) ? v ^ byte32(ok, k & 31) : v;
  };

  // the quad's Shoup table of H^4: entry n = the nibble polynomial n times
  // H^4 (8 = H^4, 4 = H^4 x, 2 = H^4 x^2, 1 = H^4 x^3); lane j builds 4j..4j+3
  {
    G4 b[4];
    b[3] = G4{{h4v.x, h4v.y, h4v.z, h4v.w}};
    b[2] = g_mulx(b[3]);
    b[1] = g_mulx(b[2]);
    b[0] = g_mulx(b[1]);
    uint32_t hi[4];
#pragma unroll
    for (int w = 0; w < 4; w++) hi[w] = bsel(j & 1, b[2].w[w], 0u) ^ bsel(j & 2, b[3].w[w], 0u);
#pragma unroll
    for (uint32_t e = 0; e < 4; e++) {
      u32x4 v;
      v.x = hi[0] ^ ((e & 1) ? b[0].w[0] : 0u) ^ ((e & 2) ? b[1].w[0] : 0u);
      v.y = hi[1] ^ ((e & 1) ? b[0].w[1] : 0u) ^ ((e & 2) ? b[1].w[1] : 0u);
      v.z = hi[2] ^ ((e & 1) ? b[0].w[2] : 0u) ^ ((e & 2) ? b[1].w[2] : 0u);
      v.w = hi[3] ^ ((e & 1) ? b[0].w[3] : 0u) ^ ((e & 2) ? b[1].w[3] : 0u);
      *(u32x4 *)&W.tab[q][4 * ((4 * j + e) ^ q)] = v;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // round keys and table are in LDS

  uint32_t hd[8];
  load_head32(src, len, hd);
  if (OB && OPEN) {
#pragma unroll
    for (int i = 0; i < 8; i++) hd[i] ^= ok[i] & range_mask(0, (int)(len < 32 ? len : 32), i);
  }
  uint32_t first, pn_len, hdr, pl, pnb[4] = {0u, 0u, 0u, 0u}, rtag[4] = {0u, 0u, 0u, 0u};
  uint64_t pn = P.pn[p];
  if (OPEN) {  // header protection off, before any in-place write
    uint32_t sample[4], m0, m1;
    load16(src + pno + 4, src + len, sample);
    load16(src + len - 16, src + len, rtag);
    if (OB) {  // (both are 16 whole bytes: pno + 4 + 16 <= len)
      uint32_t kw[4];
      keywin(ok, pno + 4, kw);
#pragma unroll
      for (int i = 0; i < 4; i++) sample[i] ^= kw[i];
      keywin(ok, len - 16, kw);
#pragma unroll
      for (int i = 0; i < 4; i++) rtag[i] ^= kw[i];
    }
    hp_mask_otf(tT, tcol, hp, sample, m0, m1);
    first = (hd[0] & 0xFFu) ^ (m0 & 0x0Fu);
    pn_len = (first & 3) + 1;
    uint64_t trunc = 0;
    for (uint32_t i = 0; i < pn_len; i++) {
      pnb[i] = hb(hd, pno + i) ^ mask_byte(m0, m1, 1 + i);
      trunc = (trunc << 8) | pnb[i];
    }
    pn = decode_pn(pn, trunc, 8 * pn_len);
    hdr = pno + pn_len;
    pl = len - 16 - hdr;  // (pno + 4 + 16 <= len)
  } else {
    first = hd[0] & 0xFFu;
    pn_len = (first & 3) + 1;
    hdr = pno + pn_len;
    pl = len - hdr;
    for (uint32_t i = 0; i < pn_len; i++) pnb[i] = hb(hd, pno + i);
  }
  uint32_t nonce[3];
  quic_nonce_iv(iv, pn, nonce);

  // GHASH blocks: A of the header (the AAD), C of ciphertext, the lengths
  const uint32_t A = (hdr + 15) / 16, C = (pl + 15) / 16, N = A + C + 1;
  const uint32_t *rk = W.rk[q], *tab = W.tab[q];
  uint32_t y[4] = {0u, 0u, 0u, 0u};
  uint32_t okp[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the key rotated to the payload start
  if (OB) key_rot(ok, hdr, okp);
  // OB open in place writes 8 bytes below where it reads.  Lanes of one step
  // in the same branch below load (one instruction) before they store, and a
  // header block's store ends below the next block's bytes.  But payload
  // block 0 is stored over header bytes [hdr - 8, hdr), which lie in the last
  // header block or the last two, and its branch may run before the header
  // branch of the same step: so a lane loads here, ahead of every store, the
  // one of those two blocks that is its own (hbl), when it comes from memory.
  uint32_t hlast[4] = {0u, 0u, 0u, 0u};
  const uint32_t hbl = A - 1 - ((A - 1 - j) & 3u);  // the lane's last header hblock
  const bool pre = OB && OPEN && hbl + 2 >= A && hbl >= 2 && hbl < A;
  if (pre) {
    load16(src + 16 * hbl, src + hdr, hlast);
    xor_half(hlast, ok, hbl & 1u);
    const int nb = (int)(hdr - 16 * hbl);
#pragma unroll
    for (int i = 0; i < 4; i++) hlast[i] &= range_mask(0, nb, i);
  }
  for (uint32_t b = j; b < N; b += 4) {
    if (b < A) {
      // the unprotected header, zero-padded; seal leaves it as it is
      // (protection is applied at the end), open writes it
      uint32_t w[4];
      if (OB && OPEN && b >= 2) {  // from memory: de-obfuscated, zero past hdr
        if (b + 2 >= A) {  // (b is hbl)
#pragma unroll
          for (int i = 0; i < 4; i++) w[i] = hlast[i];
        } else {  // (a whole block)
          load16(src + 16 * b, src + hdr, w);
          xor_half(w, ok, b & 1u);
        }
      } else {
        head_block(hd, src, 16 * b, hdr, w);
      }
      if (OPEN) {
        if (b == 0) set_byte(w, 0, first);
        for (uint32_t i = 0; i < pn_len; i++) {
          const uint32_t pos = pno + i;
          if (pos >= 16 * b && pos < 16 * b + 16) set_byte(w, pos - 16 * b, pnb[i]);
        }
      }
      ghash_absorb(y, w);
      if (OB && !OPEN) xor_half(w, ok, b & 1u);  // (store16 writes the header's bytes only)
      if (OPEN || OB || dst != src) store16(dst + 16 * b, w, hdr - 16 * b < 16 ? hdr - 16 * b : 16);
    } else if (b < A + C) {
      // payload block c: counter 2 + c; every lane of the quad loads before
      // any of them stores (one wave), and each stores where it loaded
      const uint32_t c = b - A, o = 16 * c, nb = pl - o < 16 ? pl - o : 16;
      const uint64_t S = src + hdr + o, D = dst + hdr + o;
      uint32_t x[4], ks[4] = {nonce[0], nonce[1], nonce[2], __builtin_bswap32(2u + c)};
      if (nb == 16) {
        const u32x4 v = gld<u32x4_a1>(S);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      } else {
        load16(S, S + nb, x);
      }
      if (OB && OPEN) {  // block c of the payload: half c & 1 of the rotated key
        xor_half(x, okp, c & 1u);
#pragma unroll
        for (int w = 0; w < 4; w++) x[w] &= nb == 16 ? 0xFFFFFFFFu : range_mask(0, (int)nb, w);
      }
      aes_encrypt<0, 10>(rk, tT, tcol, ks);
      uint32_t ct[4];
#pragma unroll
      for (int w = 0; w < 4; w++)
        ct[w] = (x[w] ^ ks[w]) & (nb == 16 ? 0xFFFFFFFFu : range_mask(0, (int)nb, w));
      ghash_absorb(y, OPEN ? x : ct);
      // (seal: GHASH and the sample see the ciphertext, the wire its XOR)
      if (!OPEN && c < 2) *(u32x4 *)&W.ct32[q][4 * c] = u32x4{ct[0], ct[1], ct[2], ct[3]};
      if (OB && !OPEN) xor_half(ct, okp, c & 1u);
      if (nb == 16) gst<u32x4_a1>(D, u32x4_a1{ct[0], ct[1], ct[2], ct[3]});
      else store16(D, ct, nb);
    } else {  // be64(8 * hdr) || be64(8 * pl)
      y[1] ^= 8 * hdr;
      y[2] ^= pl >> 29;
      y[3] ^= 8 * pl;
    }
    if (b + 4 < N) gmul<false>(y, tab, q);
  }
  // this lane's last block was b = j + 4 ((N - 1 - j) / 4): H^(N - b) is due
  // (a lane without a block, N < 4, holds zero)
  {
    const uint32_t bl = j + ((N - 1 - j) & ~3u), k = j < N ? N - bl : 1u;
    const u32x4 hk = gld<u32x4>(rec + offsetof(QInitRec, h) + 16ull * (k - 1));
    const G4 z = g_mul(G4{{y[0], y[1], y[2], y[3]}}, G4{{hk.x, hk.y, hk.z, hk.w}});
#pragma unroll
    for (int w = 0; w < 4; w++) y[w] = quad_xor(z.w[w]);
  }
  uint32_t tag[4] = {nonce[0], nonce[1], nonce[2], __builtin_bswap32(1u)};
  aes_encrypt<0, 10>(rk, tT, tcol, tag);  // E(K, J0)
#pragma unroll
  for (int w = 0; w < 4; w++) tag[w] ^= __builtin_bswap32(y[w]);
  if (OPEN) {
    const bool good = ((tag[0] ^ rtag[0]) | (tag[1] ^ rtag[1]) | (tag[2] ^ rtag[2]) |
                       (tag[3] ^ rtag[3])) == 0;
    if (OB && good) {
      // the datagram's bytes after this packet (coalesced packets), to the
      // offset they have in the packet: quad lane j takes bytes [64 s + 16 j,
      // + 16) of them.  In place the stores of step s land 8 bytes below its
      // loads: on the tag's bytes 8..15 (read into rtag above) and on bytes
      // that the lane below loaded in the same instruction, or a step before
      const uint32_t rem = P.in_len[p] - kSalamanderSalt - len;  // (the key kernel: >= 0)
      uint32_t okt[8];
      key_rot(ok, len, okt);
      for (uint32_t o = 16 * j; o < rem; o += 64) {
        const uint32_t nb = rem - o < 16 ? rem - o : 16;
        uint32_t x[4];
        load16(src + len + o, src + len + o + nb, x);
        xor_half(x, okt, j & 1u);  // (o / 16 is j mod 4)
        store16(dst + len + o, x, nb);
      }
    }
    if (j) return;
    P.out_len[p] = good ? len - 16 : kQEAuth;
    if (P.pn_out) P.pn_out[p] = pn;
    if (good && P.pn_offset_out) P.pn_offset_out[p] = (uint16_t)pno;
    if (good && P.consumed) P.consumed[p] = len;
    return;
  }
  // header protection: sample = (ciphertext || tag)[4 - pn_len ..][0..16)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the quad's ct32 writes
  uint32_t ct32[8];
#pragma unroll
  for (int i = 0; i < 8; i++) ct32[i] = W.ct32[q][i];
  const uint32_t so = 4 - pn_len;
  uint32_t sample[4], m0, m1;
  if (pl >= so + 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) sample[i] = __builtin_amdgcn_alignbyte(ct32[i + 1], ct32[i], so);
  } else {  // short payload: the sample reaches into the tag
    const uint32_t t8[8] = {tag[0], tag[1], tag[2], tag[3], 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; i++) sample[i] = 0u;
    for (uint32_t i = 0; i < 16; i++) {
      const uint32_t k = so + i;
      const uint32_t bb = k < pl ? byte32(ct32, k) : byte32(t8, k - pl);
      sample[i >> 2] |= bb << (8 * (i & 3));
    }
  }
  hp_mask_otf(tT, tcol, hp, sample, m0, m1);
  if (j) return;
  if (OB) {
    uint32_t kw[4];
    keywin(ok, len, kw);
#pragma unroll
    for (int i = 0; i < 4; i++) tag[i] ^= kw[i];
    const u32x2 sv = gld<u32x2>((uint64_t)P.salt + 8ull * p);
    const uint32_t s4[4] = {sv.x, sv.y, 0u, 0u};
    store16(wire, s4, kSalamanderSalt);
  }
  store16(dst + len, tag, 16);
  // (the header blocks other lanes of the quad stored have landed)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  gst<uint8_t>(dst, (uint8_t)(first ^ (m0 & 0x0Fu) ^ (ok[0] & 0xFFu)));
  for (uint32_t i = 0; i < pn_len; i++)
    gst<uint8_t>(dst + pno + i, (uint8_t)(pnb[i] ^ mask_byte(m0, m1, 1 + i) ^
                                          (OB ? byte32(ok, (pno + i) & 31) : 0u)));
  P.out_len[p] = len + 16 + (OB ? (uint32_t)kSalamanderSalt : 0u);
  if (P.pn_offset_out) P.pn_offset_out[p] = (uint16_t)pno;
}

template <bool OPEN, bool OB>
__global__ __launch_bounds__(kIBlock) void quic_initial_protect(const QInitParams P) {
  // the T-table image first (a lookup's row and column come from one v_perm,
  // the image's base is the immediate), then the waves' records
  __shared__ __attribute__((aligned(16))) uint32_t lds[kILdsWords];
  uint32_t *tT = lds;
  IWave *waves = reinterpret_cast<IWave *>(lds + 256 * 64);
  for (uint32_t i = threadIdx.x; i < 256 * 64; i += kIBlock) {
    const uint32_t v = P.t0[i >> 6];
    tT[i] = (i & 32) ? rotl(v, 8) : v;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const uint32_t tcol = 4 * (lane & 31);
  const uint64_t units = ((uint64_t)P.n + kIPpw - 1) / kIPpw;
  const uint64_t stride = (uint64_t)gridDim.x * kIWaves;
  for (uint64_t u = (uint64_t)blockIdx.x * kIWaves + wv; u < units; u += stride)
    initial_unit<OPEN, OB>(P, u * kIPpw, lane, tT, tcol, waves[wv]);
}

template <bool OPEN, bool OB>
static int launch_protect(const QInitParams *ip, hipStream_t s) {
  // the persistent grid: resident workgroups (queried once per instantiation)
  static const uint64_t cap = [] {
    int dev = 0, per_cu = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void *)quic_initial_protect<OPEN, OB>, kIBlock, 0);
    return (uint64_t)(per_cu < 1 ? 1 : per_cu) * (uint64_t)(cus < 1 ? 1 : cus);
  }();
  const uint64_t units = ((uint64_t)ip->n + kIPpw - 1) / kIPpw;
  const uint64_t want = (units + kIWaves - 1) / kIWaves;
  hipLaunchKernelGGL((quic_initial_protect<OPEN, OB>), dim3((uint32_t)(want < cap ? want : cap)),
                     dim3(kIBlock), 0, s, *ip);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sq

extern "C" int sq_launch_quic_initial(const sq::QInitParams *ip, void *stream) {
  using namespace sq;
  if (ip->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();  // (a stale error is not this launch's: sq_kernels.hip launch_k)
  const dim3 kgrid((ip->n + kIKBlock - 1) / kIKBlock);
  if (ip->obfs) hipLaunchKernelGGL((quic_initial_keys<true>), kgrid, dim3(kIKBlock), 0, s, *ip);
  else hipLaunchKernelGGL((quic_initial_keys<false>), kgrid, dim3(kIKBlock), 0, s, *ip);
  if (hipGetLastError() != hipSuccess) return -3;
  if (ip->obfs) return ip->open ? launch_protect<true, true>(ip, s) : launch_protect<false, true>(ip, s);
  return ip->open ? launch_protect<true, false>(ip, s) : launch_protect<false, false>(ip, s);
}
