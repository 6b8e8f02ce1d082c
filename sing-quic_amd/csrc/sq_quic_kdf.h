// sq_quic_kdf.h -- lane-parallel key set-up shared by the QUIC key kernels
// (sq_quic_keys.hip: 1-RTT keys derived and rolled; sq_quic_initial.hip:
// Initial keys per packet): HMAC as the two pad midstates of its key with
// the HKDF-Expand-Label messages of RFC 8446 7.1, FIPS-197 key expansion and
// one block over a plain LDS copy of the T-table, and the bitwise GF(2^128)
// multiply of SP 800-38D.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sq_bytes.h"
#include "sq_hash.h"

namespace sq {

// ---------------------------------------------------------------- HKDF

// HKDF-Expand-Label(secret, "quic <x>", "", L) message (RFC 8446 7.1) with
// HKDF-Expand's counter byte 0x01 and the hash's 0x80 pad byte:
//   u16 L | u8 11 + |x| | "tls13 quic " x | u8 0 | 0x01 | 0x80
enum { kLblKey = 0, kLblIv = 1, kLblHp = 2, kLblKu = 3 };
constexpr int label_len(int lbl) { return lbl == kLblKey ? 3 : 2; }
constexpr int info_len(int lbl) { return 16 + label_len(lbl); }  // with the counter byte
constexpr uint32_t info_byte(int lbl, int L, int k) {
  constexpr char pre[] = "tls13 quic ";
  constexpr char x[4][4] = {"key", "iv", "hp", "ku"};
  const int lx = label_len(lbl);
  if (k == 0) return (uint32_t)(L >> 8);
  if (k == 1) return (uint32_t)(L & 255);
  if (k == 2) return (uint32_t)(11 + lx);
  if (k < 14) return (uint32_t)(uint8_t)pre[k - 3];
  if (k < 14 + lx) return (uint32_t)(uint8_t)x[lbl][k - 14];
  if (k == 15 + lx) return 0x01u;
  if (k == 16 + lx) return 0x80u;
  return 0u;
}
constexpr uint32_t info_word(int lbl, int L, int i) {  // big-endian word i
  return (info_byte(lbl, L, 4 * i) << 24) | (info_byte(lbl, L, 4 * i + 1) << 16) |
         (info_byte(lbl, L, 4 * i + 2) << 8) | info_byte(lbl, L, 4 * i + 3);
}

// HMAC keyed by a secret of the hash's length, as its two pad midstates.
// Secrets and outputs are big-endian 32-bit words (8 for SHA-256, 12 for
// SHA-384; `s` and `out` are sized for the larger).
template <bool H384>
struct Prf;

template <>
struct Prf<false> {
  static constexpr int kWords = 8;
  uint32_t im[8], om[8];
  __device__ __forceinline__ void set_key(const uint32_t (&s)[12]) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = (i < 8 ? s[i] : 0u) ^ 0x36363636u;
    s2_init(im);
    s2_compress(im, m);
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] ^= 0x36363636u ^ 0x5c5c5c5cu;
    s2_init(om);
    s2_compress(om, m);
  }
  template <int LBL, int L>
  __device__ __forceinline__ void expand(uint32_t (&out)[12]) const {
    uint32_t st[8], m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = im[i];
#pragma unroll
    for (int i = 0; i < 15; i++) m[i] = info_word(LBL, L, i);
    m[15] = (64u + info_len(LBL)) * 8u;
    s2_compress(st, m);
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
};

template <>
struct Prf<true> {
  static constexpr int kWords = 12;
  uint64_t im[8], om[8];
  __device__ __forceinline__ void set_key(const uint32_t (&s)[12]) {
    uint64_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++)
      m[i] = (i < 6 ? b2_pack(s[(2 * i + 1) % 12], s[(2 * i) % 12]) : 0ull) ^ 0x3636363636363636ull;
    s5_init384(im);
    s5_compress(im, m);
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] ^= 0x3636363636363636ull ^ 0x5c5c5c5c5c5c5c5cull;
    s5_init384(om);
    s5_compress(om, m);
  }
  template <int LBL, int L>
  __device__ __forceinline__ void expand(uint32_t (&out)[12]) const {
    uint64_t st[8], m[16];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = im[i];
#pragma unroll
    for (int i = 0; i < 15; i++)
      m[i] = b2_pack(info_word(LBL, L, 2 * i + 1), info_word(LBL, L, 2 * i));
    m[15] = (128u + info_len(LBL)) * 8u;
    s5_compress(st, m);
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = st[i];
    m[6] = 0x8000000000000000ull;
#pragma unroll
    for (int i = 7; i < 15; i++) m[i] = 0ull;
    m[15] = (128u + 48u) * 8u;
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = om[i];
    s5_compress(st, m);
#pragma unroll
    for (int i = 0; i < 6; i++) {
      out[2 * i] = (uint32_t)(st[i] >> 32);
      out[2 * i + 1] = (uint32_t)st[i];
    }
  }
};

// ---------------------------------------------------------------- AES

__device__ __forceinline__ uint32_t k_rotl(uint32_t x, int n) {
  return __builtin_amdgcn_alignbit(x, x, 32 - n);
}

// the block's plain LDS copy of the T-table (t0[x] = 2s | s << 8 | s << 16 |
// 3s << 24, s = S-box(x)): one block per lane here, so bank conflicts do not
// matter as they do in the packet kernels' 32-copy image
template <uint32_t BLOCK>
__device__ __forceinline__ void stage_t0(const uint32_t *t0, uint32_t *T) {
#pragma unroll
  for (uint32_t i = threadIdx.x; i < 256; i += BLOCK) T[i] = t0[i];
  __syncthreads();
}

// SubWord on a little-endian column word: S-box = byte 1 of the T-table
__device__ __forceinline__ uint32_t sub_word(const uint32_t *T, uint32_t x) {
  const uint32_t a = T[x & 0xFFu], b = T[(x >> 8) & 0xFFu], c = T[(x >> 16) & 0xFFu],
                 d = T[x >> 24];
  return ((a >> 8) & 0xFFu) | (b & 0xFF00u) | ((c << 8) & 0xFF0000u) | ((d << 16) & 0xFF000000u);
}

constexpr uint32_t aes_rcon(int i) {  // x^i in GF(2^8)
  uint32_t r = 1;
  for (int k = 0; k < i; k++) r = ((r << 1) ^ ((r & 0x80u) ? 0x1Bu : 0u)) & 0xFFu;
  return r;
}

// FIPS-197 5.2 key expansion (NK = 4 or 8 key words) into little-endian
// column words, word 4r + c = column c of round key r; RotWord is a rotation
// right by 8 of such a word and Rcon enters its low byte.
template <int NK>
__device__ __forceinline__ void aes_expand(const uint32_t *T, const uint32_t (&key)[8],
                                           uint32_t (&rk)[4 * NK + 28]) {
#pragma unroll
  for (int i = 0; i < NK; i++) rk[i] = key[i];
#pragma unroll
  for (int i = NK; i < 4 * NK + 28; i++) {
    uint32_t t = rk[i - 1];
    if (i % NK == 0) t = sub_word(T, k_rotl(t, 24)) ^ aes_rcon(i / NK - 1);
    else if (NK == 8 && i % 8 == 4) t = sub_word(T, t);
    rk[i] = rk[i - NK] ^ t;
  }
}

// the schedule in an entry's layout: rounds 1..NR-1 rotated by 16 bits
// (sq_quic_gcm.hip aes_encrypt_n), 16-byte vector stores
template <int NK>
__device__ __forceinline__ void store_schedule(uint64_t dst, const uint32_t (&rk)[4 * NK + 28]) {
  constexpr int NR = NK + 6;
#pragma unroll
  for (int r = 0; r <= NR; r++) {
    const bool rot = r >= 1 && r < NR;
    u32x4 v;
    v.x = rot ? k_rotl(rk[4 * r], 16) : rk[4 * r];
    v.y = rot ? k_rotl(rk[4 * r + 1], 16) : rk[4 * r + 1];
    v.z = rot ? k_rotl(rk[4 * r + 2], 16) : rk[4 * r + 2];
    v.w = rot ? k_rotl(rk[4 * r + 3], 16) : rk[4 * r + 3];
    gst<u32x4>(dst + 16ull * r, v);
  }
}

// One FIPS-197 block on 4 little-endian column words with the plain
// T-table; rkey(r, k) yields round key r.  ROT: the keys of rounds 1..NR-1
// come rotated by 16 bits (an entry's stored schedule).
template <int NR, bool ROT, typename F>
__device__ __forceinline__ void aes_block_t0(const uint32_t *T, F &&rkey, uint32_t (&s)[4]) {
  uint32_t k[4], t[4];
  rkey(0, k);
#pragma unroll
  for (int c = 0; c < 4; c++) s[c] ^= k[c];
#pragma unroll
  for (int r = 1; r < NR; r++) {
    rkey(r, k);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t a0 = T[s[c] & 0xFFu], a1 = T[(s[(c + 1) & 3] >> 8) & 0xFFu];
      const uint32_t a2 = T[(s[(c + 2) & 3] >> 16) & 0xFFu], a3 = T[s[(c + 3) & 3] >> 24];
      t[c] = a0 ^ k_rotl(a1, 8) ^ k_rotl(a2, 16) ^ k_rotl(a3, 24) ^ (ROT ? k_rotl(k[c], 16) : k[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = t[c];
  }
  rkey(NR, k);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const uint32_t a0 = T[s[c] & 0xFFu], a1 = T[(s[(c + 1) & 3] >> 8) & 0xFFu];
    const uint32_t a2 = T[(s[(c + 2) & 3] >> 16) & 0xFFu], a3 = T[s[(c + 3) & 3] >> 24];
    t[c] = (((a0 >> 8) & 0xFFu) | (a1 & 0xFF00u) | ((a2 << 8) & 0xFF0000u) |
            ((a3 << 16) & 0xFF000000u)) ^ k[c];
  }
#pragma unroll
  for (int c = 0; c < 4; c++) s[c] = t[c];
}

// ---------------------------------------------------------------- GF(2^128)

// GF(2^128) element in SP 800-38D bit order as four big-endian words:
// w[0] bit 31 is the coefficient of x^0, w[3] bit 0 that of x^127.
struct G4 {
  uint32_t w[4];
};
__device__ __forceinline__ G4 g_mulx(G4 v) {  // v * x
  const uint32_t carry = 0u - (v.w[3] & 1u);
  G4 r;
  r.w[3] = __builtin_amdgcn_alignbit(v.w[2], v.w[3], 1);
  r.w[2] = __builtin_amdgcn_alignbit(v.w[1], v.w[2], 1);
  r.w[1] = __builtin_amdgcn_alignbit(v.w[0], v.w[1], 1);
  r.w[0] = (v.w[0] >> 1) ^ (carry & 0xE1000000u);
  return r;
}
__device__ __forceinline__ G4 g_xor(G4 a, G4 b) {
  return G4{{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}};
}
// SP 800-38D Algorithm 1: 128 shift-and-xor steps, x's bits from x^0 up
__device__ __forceinline__ G4 g_mul(G4 x, G4 y) {
  G4 z = {{0u, 0u, 0u, 0u}}, v = y;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t xw = x.w[j];
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
      const uint32_t m = 0u - (xw >> 31);
      xw <<= 1;
      z.w[0] ^= v.w[0] & m;
      z.w[1] ^= v.w[1] & m;
      z.w[2] ^= v.w[2] & m;
      z.w[3] ^= v.w[3] & m;
      v = g_mulx(v);
    }
  }
  return z;
}

}  // namespace sq
