// sq_quic_aes.h -- the AES rounds over the T-table image in LDS and the
// 4-bit table GHASH multiply, shared by the AES-GCM packet kernels
// (sq_quic_gcm.hip: keyring keys; sq_quic_initial.hip: Initial keys derived
// per packet).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sq_bytes.h"

namespace sq {

// ---------------------------------------------------------------- AES

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) {
  return __builtin_amdgcn_alignbit(x, x, 32 - n);
}

// readfirstlane of 32-bit values (the builtin returns int: without the
// cast a word >= 2^31 sign-extends when widened)
__device__ __forceinline__ uint32_t rfl32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}
__device__ __forceinline__ uint64_t uniform_u64(uint64_t x) {
  return ((uint64_t)rfl32((uint32_t)(x >> 32)) << 32) | (uint64_t)rfl32((uint32_t)x);
}

// Where a launch's keys live (KM): 0 one key (round keys in the kernarg
// segment, GHASH tables in LDS), 1 per-packet keyring entries in global
// memory, 2 the workgroup's staged key (GHASH tables and IV in LDS, round
// keys read wave-uniform from its keyring entry).
// round key r (4 column words); KM 2 reads them wave-uniform into SGPRs, as
// the kernarg ones are
template <int KM>
__device__ __forceinline__ void round_key(const uint32_t *rk, int r, uint32_t (&k)[4]) {
  if (KM == 1) {
    const u32x4 v = gld<u32x4>((uint64_t)(rk + 4 * r));
    k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
  } else if (KM == 2) {
    // the staged key's entry in global memory, through the constant address
    // space at a wave-uniform address: scalar loads into SGPRs (read from
    // LDS they held VGPRs and made these kernels spill)
    typedef const __attribute__((address_space(4))) uint32_t *cptr;
    const cptr c = (cptr)(uintptr_t)uniform_u64((uint64_t)(uintptr_t)(rk + 4 * r));
    k[0] = c[0]; k[1] = c[1]; k[2] = c[2]; k[3] = c[3];
  } else {
    k[0] = rk[4 * r]; k[1] = rk[4 * r + 1]; k[2] = rk[4 * r + 2]; k[3] = rk[4 * r + 3];
  }
}

// The T-table image in LDS: 256 rows of 256 bytes; row x = 32 copies of
// T0[x] then 32 copies of T1[x] = rotl8 T0[x].  Lane l reads column l & 31,
// so a ds_read_b32 (bank = word mod 32 per 32-lane half) is conflict-free.
// The byte offset of (row = byte r of s, this lane's column) is one v_perm:
// byte 0 = the lane's column offset lo = 4 (l & 31), byte 1 = s.byte r.
__device__ __forceinline__ uint32_t trow(uint32_t s, uint32_t lo, int r) {
  return __builtin_amdgcn_perm(lo, s, 0x0C0C0004u | ((uint32_t)r << 8));
}
__device__ __forceinline__ uint32_t t0at(const uint32_t *tT, uint32_t a) {
  return *(const uint32_t *)((const char *)tT + a);
}
__device__ __forceinline__ uint32_t t1at(const uint32_t *tT, uint32_t a) {
  return *(const uint32_t *)((const char *)tT + a + 128);
}

// three-input XOR in one VALU op (gfx950 v_bitop3_b32, truth table 0x96):
// the compiler emits two v_xor_b32 for a ^ b ^ c
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// FIPS-197 cipher on one block held as 4 little-endian column words.
// Round: column c = T0[s_c.b0] ^ T1[s_c+1.b1] ^ rotl16(T0[s_c+2.b2] ^
// T1[s_c+3.b3]) ^ rk (T2 = rotl16 T0, T3 = rotl16 T1; ShiftRows folded into
// the byte picks), computed as xor3(a0, a1, rotl16(xor3(a2, a3, rotr16 rk)))
// -- 3 VALU ops per column besides the 4 v_perm addresses; the key schedule
// holds rounds 1..NR-1 already rotated (sq_api.hip gcm_key).  The last
// round, NR, takes the S-box byte (T0 byte 1, T1 bytes 2 and 3) instead.
// R0 > 1: s holds the state entering round R0 (aes_ctr_n).
template <int KM, int NR, int NB, int R0 = 1>
__device__ __forceinline__ void aes_encrypt_n(const uint32_t *rk, const uint32_t *tT, uint32_t lo,
                                              uint32_t (&s)[NB][4]) {
  uint32_t k[4];
  if (R0 == 1) {
    round_key<KM>(rk, 0, k);
#pragma unroll
    for (int q = 0; q < NB; q++)
#pragma unroll
      for (int c = 0; c < 4; c++) s[q][c] ^= k[c];
  }
#pragma unroll
  for (int r = R0; r < NR; r++) {
    uint32_t kr[4];  // (rotated by 16 in the key schedule)
    round_key<KM>(rk, r, kr);
    uint32_t t[NB][4];
#pragma unroll
    for (int q = 0; q < NB; q++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t a0 = t0at(tT, trow(s[q][c], lo, 0));
        const uint32_t a1 = t1at(tT, trow(s[q][(c + 1) & 3], lo, 1));
        const uint32_t a2 = t0at(tT, trow(s[q][(c + 2) & 3], lo, 2));
        const uint32_t a3 = t1at(tT, trow(s[q][(c + 3) & 3], lo, 3));
        t[q][c] = xor3(a0, a1, rotl(xor3(a2, a3, kr[c]), 16));
      }
#pragma unroll
    for (int q = 0; q < NB; q++)
#pragma unroll
      for (int c = 0; c < 4; c++) s[q][c] = t[q][c];
  }
  round_key<KM>(rk, NR, k);
  uint32_t t[NB][4];
#pragma unroll
  for (int q = 0; q < NB; q++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t a0 = t0at(tT, trow(s[q][c], lo, 0));
      const uint32_t a1 = t0at(tT, trow(s[q][(c + 1) & 3], lo, 1));
      const uint32_t a2 = t1at(tT, trow(s[q][(c + 2) & 3], lo, 2));
      const uint32_t a3 = t1at(tT, trow(s[q][(c + 3) & 3], lo, 3));
      // S-box bytes: T0 byte 1 (a0, a1), T1 bytes 2 and 3 (a2, a3), two v_perm
      // into complementary bytes, then one three-input XOR with the key
      t[q][c] = xor3(__builtin_amdgcn_perm(a1, a0, 0x0C0C0501u),
                     __builtin_amdgcn_perm(a3, a2, 0x07020C0Cu), k[c]);
    }
#pragma unroll
  for (int q = 0; q < NB; q++)
#pragma unroll
    for (int c = 0; c < 4; c++) s[q][c] = t[q][c];
}

template <int KM, int NR>
__device__ __forceinline__ void aes_encrypt(const uint32_t *rk, const uint32_t *tT, uint32_t lo,
                                            uint32_t (&s)[4]) {
  uint32_t b[1][4] = {{s[0], s[1], s[2], s[3]}};
  aes_encrypt_n<KM, NR, 1>(rk, tT, lo, b);
#pragma unroll
  for (int c = 0; c < 4; c++) s[c] = b[0][c];
}

// ---------------------------------------------------------------- GHASH

// x <- x * H^k in GF(2^128) (SP 800-38D bit order), x as big-endian words
// (x[0] = bytes 0..3).  tab = the 16-entry 4-bit table of H^k; nibbles are
// consumed from the low end of the 128-bit integer, each step multiplying
// the accumulator by x^4 (shift right 4, fold the 4 bits shifted out back
// with the reduction polynomial).  Entry n of table k-1 is stored in slot
// n ^ sw, sw = (k-1) & 15: lanes multiplying by different powers then read
// different 16-byte slots of the bank row for the same nibble (no
// ds_read_b128 bank conflicts).
// One word (8 nibbles) at a time: its table reads depend only on x, so they
// are issued back to back (4 in flight); the shifts then run with the
// fold deferred to the end of the word -- the bits shifted out collect in z4
// (fold bits enter z0 at bit 21 or above and cannot reach z3's low nibble
// within 8 shifts), and fold(u) = u ^ u>>1 ^ u>>2 ^ u>>7 over z0:z1, the
// 4-bit fold (rem<<28 ^ rem<<27 ^ rem<<26 ^ rem<<21) applied to 32 bits at
// once.
template <bool GLOBAL>
__device__ __forceinline__ void gmul(uint32_t (&x)[4], const uint32_t *tab, uint32_t sw) {
  uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
  uint32_t w = x[3], w2 = x[2], w1 = x[1], w0 = x[0];
  const char *t = (const char *)tab;
  const uint32_t sw16 = sw << 4;
  // one word per iteration, kept rolled (unrolled, the compiler hoists every
  // word's reads and spills)
#pragma unroll 1
  for (int i = 0; i < 4; i++) {
    const uint32_t w4 = w << 4;
    uint32_t z4 = 0;
#pragma unroll
    for (int h = 0; h < 8; h += 4) {  // (4 reads in flight: 8 made the kernels spill)
      u32x4 e[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int jj = h + j;
        const uint32_t off = ((((jj & 1) ? w : w4) >> (8 * (jj >> 1))) & 0xF0u) ^ sw16;
        if (GLOBAL) e[j] = gld<u32x4>((uint64_t)(t + off));
        else e[j] = *(const u32x4 *)(t + off);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (i | h | j) {
          z4 = __builtin_amdgcn_alignbit(z3, z4, 4);
          z3 = __builtin_amdgcn_alignbit(z2, z3, 4);
          z2 = __builtin_amdgcn_alignbit(z1, z2, 4);
          z1 = __builtin_amdgcn_alignbit(z0, z1, 4);
          z0 >>= 4;
        }
        z0 ^= e[j].x; z1 ^= e[j].y; z2 ^= e[j].z; z3 ^= e[j].w;
      }
    }
    z0 = xor3(z0, xor3(z4, z4 >> 1, z4 >> 2), z4 >> 7);
    z1 ^= xor3(z4 << 31, z4 << 30, z4 << 25);
    w = w2;
    w2 = w1;
    w1 = w0;
  }
  x[0] = z0; x[1] = z1; x[2] = z2; x[3] = z3;
}

// y ^= 16 bytes held as little-endian words
__device__ __forceinline__ void ghash_absorb(uint32_t (&y)[4], const uint32_t (&m)[4]) {
#pragma unroll
  for (int w = 0; w < 4; w++) y[w] ^= __builtin_bswap32(m[w]);
}

}  // namespace sq
