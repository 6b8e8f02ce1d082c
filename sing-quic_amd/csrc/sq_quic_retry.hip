// sq_quic_retry.hip -- gfx950 QUIC v1 Retry packets and the validation of the
// address-validation tokens they carry (RFC 9000 8.1.2, 17.2.5; RFC 9001 5.8).
//
// Replaces, for a whole ragged batch per launch, what a quic-go listener does
// per unvalidated Initial on the host
//   transport.go  handleInitial -> sendRetry / validateToken
//   internal/handshake/retry.go  GetRetryIntegrityTag
//   internal/handshake/token_generator.go  NewRetryToken / DecodeToken
// (quic-go v0.52.0-beta.1, go.mod:7; not in the reference tree), and under
// Hysteria2 the Salamander pass on both sides of it: the Initial arrives
// obfuscated, the Retry leaves obfuscated.
//
// What sets this work apart from the Initial and 1-RTT kernels: every
// datagram uses the same two keys (the endpoint's token key and the public
// Retry integrity key), so no key is expanded and no GHASH table is built per
// packet, and the messages are tiny (at most 3 AES blocks and 16 GHASH
// blocks) but byte-ragged: three connection-id lengths move every field.
//
// Work decomposition, one launch: quic_retry<CHECK, OB>, 512 lanes (8 waves)
// per workgroup, a persistent grid, a wave takes 64 datagrams at a time, one
// lane each.  LDS per workgroup: the 64 KiB T-table image, two 256-byte 4-bit
// tables (H of the token key, copied from the keyring's device entry; H of the
// Retry key, made once on the host), and one 176-byte row per lane:
//   row [0, 160)   the lane's assembly area, 16-byte aligned
//   row [160, 176) the output record: destination, packet start, length
// 176 = 11 x 16: rows of consecutive lanes start 12 banks apart, so the eight
// lanes of a 16-byte LDS access hit eight different bank quads.
// Fields are put into the row at their byte positions with byte-aligned
// stores, lowest address first (a field's padding is overwritten by the
// next), and read back as aligned 16-byte GHASH blocks: the raggedness is
// resolved by the LDS address, not by shifting registers.  The row is used
// twice: first for the token's AAD (addr || cid_len || cid, 39 bytes) and
// plaintext (issued_at || odcid_len || odcid, 25 bytes), then, retry, for the
// pseudo-packet odcid_len || odcid || Retry header || token, whose tag lands
// behind it.  GHASH over it uses the constant Retry table and ends with the
// XOR of the constant E_K(J0): the Retry tag takes no AES at all; the token
// takes three blocks (J0 and two counters) in one interleaved pass under
// round keys read wave-uniform from the kernarg segment.
// Output: the wave copies its 64 packets out of the rows, eight lanes per
// packet, 16 bytes per lane, so a packet leaves as one contiguous run of
// 16-byte stores.  Under Salamander (OB) the lane derives the datagram's key
// before parsing, and for a Retry a second key from salt[i], which it XORs
// over its row (rotated once to the packet's start) before the copy.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/sqobfs.h"
#include "sq_bytes.h"
#include "sq_hash.h"
#include "sq_internal.h"
#include "sq_obfs_key.h"
#include "sq_quic.h"
#include "sq_quic_aes.h"

namespace sq {

constexpr uint32_t kYBlock = 512;  // 8 waves: two per SIMD
constexpr uint32_t kYWaves = kYBlock / kWave;
constexpr uint32_t kRow = 160, kRowStride = 176;
constexpr uint32_t kTokLen = SQOBFS_QUIC_RETRY_TOKEN_LEN, kTokMax = SQOBFS_QUIC_RETRY_TOKEN_MAX;
constexpr uint32_t kTokAad = 39, kTokPlain = 25;
constexpr uint32_t kYLdsWords = 256 * 64 + 2 * 64 + kYBlock * kRowStride / 4;
static_assert(kYLdsWords * 4 <= 160 * 1024, "the LDS image exceeds gfx950's 160 KiB per workgroup");
// the longest pseudo-packet and its tag fit the row
static_assert(1 + kMaxCid + 6 + kMaxCid + 1 + kMaxCid + kTokMax + 16 <= kRow, "row");
static_assert(6 + kMaxCid + 1 + kMaxCid + kTokMax + 16 == SQOBFS_QUIC_RETRY_MAX, "Retry packet");
static_assert(12 + kTokPlain + 16 == kTokLen, "token");

// LDS and global accesses at byte-aligned addresses
#define SQ_LDS __attribute__((address_space(3)))
typedef SQ_LDS char *lrow;
typedef uint32_t u32_a1 __attribute__((aligned(1)));
typedef uint16_t u16_a1 __attribute__((aligned(1)));
__device__ __forceinline__ void lst32(lrow p, uint32_t v) { *(SQ_LDS u32_a1 *)p = v; }
__device__ __forceinline__ void lst8(lrow p, uint32_t v) { *(SQ_LDS uint8_t *)p = (uint8_t)v; }
__device__ __forceinline__ void lst128(lrow p, u32x4 v) { *(SQ_LDS u32x4 *)p = v; }  // 16-aligned
__device__ __forceinline__ void lld128(lrow p, uint32_t (&w)[4]) {
  const u32x4 v = *(const SQ_LDS u32x4 *)p;
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ uint32_t gld32(uint64_t a) { return *(const SQ_GLOBAL u32_a1 *)a; }
__device__ __forceinline__ void gst32(uint64_t a, uint32_t v) { *(SQ_GLOBAL u32_a1 *)a = v; }

// a 20-byte field (5 words) at byte p of the row
__device__ __forceinline__ void lst_cid(lrow p, const uint32_t (&c)[5]) {
#pragma unroll
  for (int j = 0; j < 5; j++) lst32(p + 4 * j, c[j]);
}

// The token's AAD in row [0, 48): addr[i] (18) || cl || cid zero-padded to 20,
// zero to the block's end.
__device__ __forceinline__ void token_aad(lrow row, uint64_t addr, uint32_t cl,
                                          const uint32_t (&cid)[5]) {
  lst128(row + 32, u32x4{0u, 0u, 0u, 0u});
  lst128(row, u32x4{gld32(addr), gld32(addr + 4), gld32(addr + 8), gld32(addr + 12)});
  lst32(row + 16, (uint32_t)*(const SQ_GLOBAL u16_a1 *)(addr + 16) | (cl << 16));
  lst_cid(row + 19, cid);  // (ends at byte 39)
}

// AES-128-GCM of a library token under the endpoint's key: nonce = iv ^ nw,
// AAD = row [0, 39), x = the 25 bytes (zero past them) of ciphertext (DEC) or
// plaintext; x comes back as the other, tag as the tag it should carry.
template <bool DEC>
__device__ __forceinline__ void token_gcm(const QRetryParams &P, const uint32_t *tT, uint32_t tcol,
                                          const uint32_t *htok, lrow row, const uint32_t (&nw)[3],
                                          uint32_t (&x)[2][4], uint32_t (&tag)[4]) {
  uint32_t s[3][4];  // E(J0) and the keystream of counters 2, 3
#pragma unroll
  for (int q = 0; q < 3; q++) {
#pragma unroll
    for (int w = 0; w < 3; w++) s[q][w] = P.tiv[w] ^ nw[w];
    s[q][3] = __builtin_bswap32(1u + q);
  }
  aes_encrypt_n<0, 10, 3>(P.trk, tT, tcol, s);
  uint32_t y[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
  for (uint32_t b = 0; b < (kTokAad + 15) / 16; b++) {
    uint32_t w[4];
    lld128(row + 16 * b, w);
    ghash_absorb(y, w);
    gmul<false>(y, htok, 0);
  }
#pragma unroll
  for (int q = 0; q < 2; q++) {
    uint32_t o[4];
#pragma unroll
    for (int w = 0; w < 4; w++)
      o[w] = (x[q][w] ^ s[1 + q][w]) & range_mask(0, (int)kTokPlain - 16 * q, w);
    if (DEC) ghash_absorb(y, x[q]);  // (the ciphertext is hashed)
    else ghash_absorb(y, o);
    gmul<false>(y, htok, 0);
#pragma unroll
    for (int w = 0; w < 4; w++) x[q][w] = o[w];
  }
  y[1] ^= 8 * kTokAad;  // be64(8 * 39) || be64(8 * 25)
  y[3] ^= 8 * kTokPlain;
  gmul<false>(y, htok, 0);
#pragma unroll
  for (int w = 0; w < 4; w++) tag[w] = s[0][w] ^ __builtin_bswap32(y[w]);
}

// w ^= half `odd` of the 32-byte key k
__device__ __forceinline__ void xor_key_half(uint32_t (&w)[4], const uint32_t (&k)[8], bool odd) {
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] ^= bsel(odd, k[4 + i], k[i]);
}

// Datagram i of the batch, in the lane's row.  Retry: leaves the packet in the
// row and its output record behind it.
template <bool CHECK, bool OB>
__device__ __forceinline__ void retry_lane(const QRetryParams &P, uint32_t i, const uint32_t *tT,
                                           uint32_t tcol, const uint32_t *htok,
                                           const uint32_t *rtab, lrow row) {
  uint64_t src = (uint64_t)P.in + P.in_off[i];
  uint32_t len = P.in_len[i];
  uint32_t ok[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the datagram's Salamander key
  if (OB) {  // as quic_initial_keys: salt8 || packet ^ K
    if (len >= (uint32_t)kSalamanderSalt && len <= kQMaxPacket) {
      uint32_t osalt[4];
      load16(src, src + kSalamanderSalt, osalt);
      salamander_key(P.opsk, osalt, ok);
      src += kSalamanderSalt;
      len -= kSalamanderSalt;
    } else {
      len = 0;
    }
  }
  uint32_t err = len == 0 || len > kQMaxPacket ? kQEShort : 0u;
  uint32_t hd[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, pno = 0;
  uint64_t length = 0;
  if (!err) {
    load_head32(src, len, hd);
    if (OB) {
#pragma unroll
      for (int j = 0; j < 8; j++) hd[j] ^= ok[j] & range_mask(0, (int)(len < 32 ? len : 32), j);
    }
    err = parse_initial<OB>(hd, src, len, 1u, pno, length, ok);
  }
  if (err) {
    if (CHECK) P.status[i] = (uint8_t)SQOBFS_QUIC_TOKEN_EHEADER;
    else P.out_len[i] = err;
    return;
  }
  // the header is inside the packet: DCID at byte 6 (within the head), then
  // scid_len || SCID || token length (varint) || token
  const uint32_t dl = (hd[1] >> 8) & 0xFFu, sl = byte32(hd, 6 + dl);
  uint32_t d[5];
#pragma unroll
  for (int j = 0; j < 5; j++)
    d[j] = __builtin_amdgcn_alignbyte(hd[j + 2], hd[j + 1], 2) & range_mask(0, (int)dl, j);
  const uint64_t addr = (uint64_t)P.addr + 18ull * i;

  if (CHECK) {
    auto hb = [&](uint32_t k) -> uint32_t {
      const uint32_t b = head_byte(hd, src, k);
      return (OB && k >= 32) ? b ^ byte32(ok, k & 31) : b;
    };
    uint32_t p = 7 + dl + sl;
    const uint32_t b0 = hb(p), nb = 1u << (b0 >> 6);
    uint64_t tok = b0 & 0x3Fu;
    for (uint32_t k = 1; k < nb; k++) tok = (tok << 8) | hb(p + k);
    p += nb;
    if (tok != kTokLen) {
      P.status[i] = (uint8_t)(tok ? SQOBFS_QUIC_TOKEN_FOREIGN : SQOBFS_QUIC_TOKEN_NONE);
      return;
    }
    // nonce12 || C25 || T16 at packet byte p (the parser: inside the packet)
    const uint64_t t = src + p, te = t + kTokLen;
    uint32_t nw4[4], x[2][4], rtag[4], tag[4];
    load16(t, te, nw4);
    load16(t + 12, te, x[0]);
    load16(t + 28, t + 12 + kTokPlain, x[1]);
    load16(t + 12 + kTokPlain, te, rtag);
    if (OB) {
      uint32_t kw[4];
      keywin(ok, p, kw);
#pragma unroll
      for (int w = 0; w < 4; w++) nw4[w] ^= kw[w];
      keywin(ok, p + 12, kw);
#pragma unroll
      for (int w = 0; w < 4; w++) x[0][w] ^= kw[w];
      keywin(ok, p + 28, kw);
#pragma unroll
      for (int w = 0; w < 4; w++) x[1][w] = (x[1][w] ^ kw[w]) & range_mask(0, (int)kTokPlain - 16, w);
      keywin(ok, p + 12 + kTokPlain, kw);
#pragma unroll
      for (int w = 0; w < 4; w++) rtag[w] ^= kw[w];
    }
    const uint32_t nw[3] = {nw4[0], nw4[1], nw4[2]};
    token_aad(row, addr, dl, d);  // the Initial answers a Retry: its DCID is the Retry's SCID
    token_gcm<true>(P, tT, tcol, htok, row, nw, x, tag);
    if (((tag[0] ^ rtag[0]) | (tag[1] ^ rtag[1]) | (tag[2] ^ rtag[2]) | (tag[3] ^ rtag[3])) != 0) {
      P.status[i] = (uint8_t)SQOBFS_QUIC_TOKEN_BAD;
      return;
    }
    // issued_at (be32) || odcid_len || odcid[20]
    const uint32_t issued = __builtin_bswap32(x[0][0]);
    const uint32_t pw[7] = {x[0][0], x[0][1], x[0][2], x[0][3], x[1][0], x[1][1], x[1][2]};
#pragma unroll
    for (int j = 0; j < 5; j++)
      gst32((uint64_t)P.odcid_out + 20ull * i + 4 * j,
            __builtin_amdgcn_alignbyte(pw[j + 2], pw[j + 1], 1));
    P.odcid_len_out[i] = (uint8_t)pw[1];
    if (P.issued_at_out) P.issued_at_out[i] = issued;
    P.status[i] = (uint8_t)((uint32_t)(P.now - issued) > P.max_age ? SQOBFS_QUIC_TOKEN_EXPIRED
                                                                  : SQOBFS_QUIC_TOKEN_OK);
    return;
  }

  // ---- retry
  const uint32_t rl = P.rscid_len;
  uint32_t r[5];
#pragma unroll
  for (int j = 0; j < 5; j++)
    r[j] = gld32((uint64_t)P.rscid + 20ull * i + 4 * j) & range_mask(0, (int)rl, j);
  // the token: the caller's 64 bytes, or nonce12 || C25 || T16 made here
  uint32_t tk[16], tl, nw[3], x[2][4], tag[4];
  if (P.token) {
    tl = P.token_len[i];
    tl = tl < kTokMax ? tl : kTokMax;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u32x4 v = gld<u32x4>((uint64_t)P.token + 64ull * i + 16 * q);
      tk[4 * q] = v.x; tk[4 * q + 1] = v.y; tk[4 * q + 2] = v.z; tk[4 * q + 3] = v.w;
    }
  } else {
    tl = kTokLen;
#pragma unroll
    for (int w = 0; w < 3; w++) nw[w] = gld32((uint64_t)P.nonce + 12ull * i + 4 * w);
    token_aad(row, addr, rl, r);
    // the plaintext in row [48, 73), zero to byte 80
    lst128(row + 64, u32x4{0u, 0u, 0u, 0u});
    lst32(row + 48, __builtin_bswap32(P.now));
    lst8(row + 52, dl);
    lst_cid(row + 53, d);
    lld128(row + 48, x[0]);
    lld128(row + 64, x[1]);
    token_gcm<false>(P, tT, tcol, htok, row, nw, x, tag);
  }
  // the client's SCID: sl bytes at packet byte 7 + dl, up to byte 47
  uint32_t sc[5] = {0u, 0u, 0u, 0u, 0u};
  if (sl) {
    const uint64_t sa = src + 7 + dl;
    uint32_t a[4], b[4] = {0u, 0u, 0u, 0u};
    load16(sa, sa + sl, a);
    if (sl > 16) load16(sa + 16, sa + sl, b);
    if (OB) {
      uint32_t kw[4];
      keywin(ok, 7 + dl, kw);
#pragma unroll
      for (int w = 0; w < 4; w++) a[w] ^= kw[w];
      keywin(ok, 7 + dl + 16, kw);
      b[0] ^= kw[0];
    }
    sc[0] = a[0]; sc[1] = a[1]; sc[2] = a[2]; sc[3] = a[3]; sc[4] = b[0];
  }
  // the pseudo-packet (RFC 9001 5.8), lowest address first:
  //   dl | ODCID | 0xF0 | 00000001 | sl | SCID | rl | rscid | token
  const uint32_t R = 1 + dl;     // the Retry packet starts here
  const uint32_t Q = R + 6 + sl;
  const uint32_t T = Q + 1 + rl, L = T + tl;  // (L <= 132)
  lst8(row, dl);
  lst_cid(row + 1, d);
  lst8(row + R, 0xF0u);
  lst32(row + R + 1, 0x01000000u);
  lst8(row + R + 5, sl);
  lst_cid(row + R + 6, sc);
  lst8(row + Q, rl);
  lst_cid(row + Q + 1, r);
  if (P.token) {
#pragma unroll
    for (int w = 0; w < 16; w++) lst32(row + T + 4 * w, tk[w]);
  } else {  // (C's last word holds one byte: the tag follows at token byte 37)
#pragma unroll
    for (int w = 0; w < 3; w++) lst32(row + T + 4 * w, nw[w]);
#pragma unroll
    for (int w = 0; w < 7; w++) lst32(row + T + 12 + 4 * w, x[w >> 2][w & 3]);
#pragma unroll
    for (int w = 0; w < 4; w++) lst32(row + T + 12 + kTokPlain + 4 * w, tag[w]);
  }
#pragma unroll
  for (int w = 0; w < 4; w++) lst32(row + L + 4 * w, 0u);  // the last block's padding
  // tag = GHASH_H(pseudo-packet || lengths) ^ E_K(J0): the plaintext is empty
  uint32_t y[4] = {0u, 0u, 0u, 0u};
  const uint32_t nblk = (L + 15) / 16;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; b++) {
    uint32_t w[4];
    lld128(row + 16 * b, w);
    ghash_absorb(y, w);
    gmul<false>(y, rtab, 0);
  }
  y[1] ^= 8 * L;
  gmul<false>(y, rtab, 0);
#pragma unroll
  for (int w = 0; w < 4; w++) lst32(row + L + 4 * w, P.ekj0[w] ^ __builtin_bswap32(y[w]));
  const uint32_t plen = L + 16 - R;
  uint64_t dst = (uint64_t)P.out + P.out_off[i];
  if (OB) {
    // the Retry datagram's own key, from salt[i]; row byte b gets key byte
    // (b - R) & 31: rotated once, then half b / 16 & 1 per aligned block
    const u32x2 sv = gld<u32x2>((uint64_t)P.salt + 8ull * i);
    const uint32_t s4[4] = {sv.x, sv.y, 0u, 0u};
    uint32_t k2[8], ka[4], kb[4];
    salamander_key(P.opsk, s4, k2);
    keywin(k2, 32 - (R & 31), ka);
    keywin(k2, 48 - (R & 31), kb);
    const uint32_t kr[8] = {ka[0], ka[1], ka[2], ka[3], kb[0], kb[1], kb[2], kb[3]};
#pragma unroll 1
    for (uint32_t b = R / 16; b < (L + 16 + 15) / 16; b++) {
      uint32_t w[4];
      lld128(row + 16 * b, w);
      xor_key_half(w, kr, b & 1u);
      lst128(row + 16 * b, u32x4{w[0], w[1], w[2], w[3]});
    }
    store16(dst, s4, kSalamanderSalt);
    dst += kSalamanderSalt;
  }
  lst128(row + kRow, u32x4{(uint32_t)dst, (uint32_t)(dst >> 32), R, plen});
  P.out_len[i] = plen + (OB ? (uint32_t)kSalamanderSalt : 0u);
}

template <bool CHECK, bool OB>
__global__ __launch_bounds__(kYBlock) void quic_retry(const QRetryParams P) {
  // the T-table image first (as quic_initial_protect), the two tables of H,
  // then the lanes' rows
  __shared__ __attribute__((aligned(16))) uint32_t lds[kYLdsWords];
  uint32_t *tT = lds, *htok = lds + 256 * 64, *rtab = htok + 64;
  for (uint32_t i = threadIdx.x; i < 256 * 64; i += kYBlock) {
    const uint32_t v = P.t0[i >> 6];
    tT[i] = (i & 32) ? rotl(v, 8) : v;
  }
  if (threadIdx.x < 64) htok[threadIdx.x] = P.htok ? P.htok[threadIdx.x] : 0u;
  else if (threadIdx.x < 128) htok[threadIdx.x] = P.rtab[threadIdx.x - 64];
  __syncthreads();
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const uint32_t tcol = 4 * (lane & 31);
  const lrow rows = (lrow)(char *)(rtab + 64) + wv * kWave * kRowStride;
  const lrow row = rows + lane * kRowStride;
  const uint64_t units = ((uint64_t)P.n + kWave - 1) / kWave;
  const uint64_t stride = (uint64_t)gridDim.x * kYWaves;
  for (uint64_t u = (uint64_t)blockIdx.x * kYWaves + wv; u < units; u += stride) {
    const uint64_t i = u * kWave + lane;
    if (!CHECK) lst128(row + kRow, u32x4{0u, 0u, 0u, 0u});  // nothing to copy
    if (i < P.n) retry_lane<CHECK, OB>(P, (uint32_t)i, tT, tcol, htok, rtab, row);
    if (CHECK) continue;
    // the wave's packets leave the rows: 8 lanes per packet, 16 bytes each
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (uint32_t t = lane; t < 8 * kWave; t += kWave) {
      const lrow pr = rows + (t >> 3) * kRowStride;
      uint32_t m[4];
      lld128(pr + kRow, m);
      const uint32_t o = 16 * (t & 7), plen = m[3];
      if (o >= plen) continue;
      const uint32_t a = m[2] + o;  // (a < R + plen <= 148: block a / 16 + 1 <= 9 when read)
      uint32_t lo4[4], hi4[4] = {0u, 0u, 0u, 0u}, v[4];
      lld128(pr + (a & ~15u), lo4);
      if ((a >> 4) < kRow / 16 - 1) lld128(pr + (a & ~15u) + 16, hi4);
      funnel(lo4, hi4, a & 15u, v);
      const uint64_t D = (((uint64_t)m[1] << 32) | m[0]) + o;
      if (plen - o >= 16) gst<u32x4_a1>(D, u32x4_a1{v[0], v[1], v[2], v[3]});
      else store16(D, v, plen - o);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // before the rows are written again
    __builtin_amdgcn_wave_barrier();
  }
}

template <bool CHECK, bool OB>
static int launch_retry(const QRetryParams *rp, hipStream_t s) {
  // the persistent grid: resident workgroups (queried once per instantiation)
  static const uint64_t cap = [] {
    int dev = 0, per_cu = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void *)quic_retry<CHECK, OB>, kYBlock, 0);
    return (uint64_t)(per_cu < 1 ? 1 : per_cu) * (uint64_t)(cus < 1 ? 1 : cus);
  }();
  const uint64_t units = ((uint64_t)rp->n + kWave - 1) / kWave;
  const uint64_t want = (units + kYWaves - 1) / kYWaves;
  hipLaunchKernelGGL((quic_retry<CHECK, OB>), dim3((uint32_t)(want < cap ? want : cap)),
                     dim3(kYBlock), 0, s, *rp);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace sq

extern "C" int sq_launch_quic_retry(int check, int obfs, const sq::QRetryParams *rp,
                                    void *stream) {
  using namespace sq;
  if (rp->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();  // (a stale error is not this launch's: sq_kernels.hip launch_k)
  if (check) return obfs ? launch_retry<true, true>(rp, s) : launch_retry<true, false>(rp, s);
  return obfs ? launch_retry<false, true>(rp, s) : launch_retry<false, false>(rp, s);
}
