// sq_quic_keys.hip -- gfx950 QUIC key schedule: 1-RTT keys derived and rolled
// on the device (RFC 9001 5.1 and 6), and the Key Phase resolver.
//
// Replaces, for many connections per launch, what quic-go does once per
// connection and per key update on the host
//   internal/handshake/updatable_aead.go   rollKeys / getNextTrafficSecret
//   internal/handshake/hkdf.go             hkdfExpandLabel
//   internal/handshake/aead.go / header_protector.go   key set-up
// (quic-go v0.52.0-beta.1, go.mod:7; reached from the reference through
// quic.go:47-102; not in the reference tree).  The algorithms are RFC 5869
// HKDF-Expand with RFC 8446 7.1 labels over HMAC-SHA-256 / HMAC-SHA-384
// (FIPS 180-4, RFC 2104), FIPS-197 key expansion and the GHASH tables of
// sq_quic_gcm.hip (layout: QuicGcmKeyDev, sq_internal.h).
//
// Keyring model: connection c's generation g lives in entry 2c + (g & 1), so
// a packet's Key Phase bit is the low bit of its entry index, and the keyring
// keeps each connection's newest secret and generation on the device.
//
// Work decomposition:
//   1. quic_derive: one lane per connection.  The HMAC inner and outer pad
//      midstates are compressed once per secret and shared by its labels;
//      every Expand-Label message (at most 19 B with the counter byte) fits
//      the one block after the pad, so a label costs two compressions.  A
//      new connection derives generation 0 (key, iv, hp), "quic ku", then
//      generation 1 (key, iv); a key update derives "quic ku" from the stored
//      secret, then key and iv into the entry of the generation before it.
//      For ChaCha20-Poly1305 the result is the QuicKeyDev words.  For the GCM
//      suites the lane goes on: both AES key expansions (S-box = byte 1 of
//      the T-table, 1 KiB in LDS), stored in the entry's layout (rounds
//      1..NR-1 rotated by 16 bits), and H = E(K, 0^128).
//   2. quic_gcm_tables: one wave per entry, lane l owns row l of the entry's
//      64 table rows of 256 B.  Lanes 0-31 (hpos row j): H x^(4 (31 - j)) by
//      up to 124 multiply-by-x steps.  Lanes 32-63 (htab row pw): H^(4 (pw +
//      1)) by square-and-multiply on H^4 (128 shift-and-xor steps per
//      product, on four 32-bit words).  Both halves then form the 16 nibble
//      multiples from four basis values and write them as 16-byte vector
//      stores (htab in slot n ^ (pw & 15)).
//   3. quic_key_phase: one lane per packet computes byte 0 of the
//      header-protection mask (one ChaCha20 block, or one AES block under the
//      entry's hp schedule with a plain LDS copy of the T-table) and writes
//      the entry index with its low bit set to the packet's Key Phase bit.
//      OB (sqobfs_quic_key_phase_salamander): the batch holds Hysteria2 wire
//      datagrams, salt8 || packet ^ K.  The lane derives K = BLAKE2b-256(psk
//      || salt) itself (the resolver runs before open, so no other kernel has
//      made it yet) and de-obfuscates the two things it reads: the first
//      byte with K[0], and the sample with K rotated to its packet offset.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "sq_bytes.h"
#include "sq_hash.h"
#include "sq_internal.h"
#include "sq_obfs_key.h"
#include "sq_quic.h"
#include "sq_quic_kdf.h"
#include "sqobfs.h"

namespace sq {

constexpr uint32_t kKBlock = 64;   // derive: one wave per workgroup (spreads few connections)
constexpr uint32_t kTBlock = 256;  // tables: 4 waves = 4 entries per workgroup
constexpr uint32_t kPBlock = 256;  // key phase

// ---------------------------------------------------------------- derive

// One generation's key and iv (and, HP, the connection's hp) from the
// midstates of its secret, into keyring entry e; hp also into entry e ^ 1
// (both entries of a connection carry the same header protection).
template <uint32_t SUITE, bool HP>
__device__ __forceinline__ void derive_entry(const QKeysParams &P,
                                             const Prf<SUITE == SQOBFS_QUIC_AES_256_GCM> &prf,
                                             const uint32_t *T, uint32_t e) {
  constexpr int KL = SUITE == SQOBFS_QUIC_AES_128_GCM ? 16 : 32;
  uint32_t d[12], key[8], iv[3];
  prf.template expand<kLblKey, KL>(d);
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = __builtin_bswap32(d[i]);
  prf.template expand<kLblIv, 12>(d);
#pragma unroll
  for (int i = 0; i < 3; i++) iv[i] = __builtin_bswap32(d[i]);
  if (SUITE == SQOBFS_QUIC_CHACHA20_POLY1305) {
    const uint64_t a = (uint64_t)(P.keys + e);
    gst<u32x4>(a, u32x4{key[0], key[1], key[2], key[3]});
    gst<u32x4>(a + 16, u32x4{key[4], key[5], key[6], key[7]});
    gst<u32x2>(a + 32, u32x2{iv[0], iv[1]});
    gst<uint32_t>(a + 40, iv[2]);
    if (HP) {  // words 11..18, then the pad word
      prf.template expand<kLblHp, KL>(d);
      uint32_t hp[8];
#pragma unroll
      for (int i = 0; i < 8; i++) hp[i] = __builtin_bswap32(d[i]);
#pragma unroll
      for (int o = 0; o < 2; o++) {
        const uint64_t b = (uint64_t)(P.keys + (e ^ (uint32_t)o));
        gst<uint32_t>(b + 44, hp[0]);
        gst<u32x4>(b + 48, u32x4{hp[1], hp[2], hp[3], hp[4]});
        gst<u32x4>(b + 64, u32x4{hp[5], hp[6], hp[7], 0u});
      }
    }
  } else {
    constexpr int NK = KL / 4;
    uint32_t rk[4 * NK + 28];
    if (HP) {
      prf.template expand<kLblHp, KL>(d);
      uint32_t hp[8];
#pragma unroll
      for (int i = 0; i < 8; i++) hp[i] = __builtin_bswap32(d[i]);
      aes_expand<NK>(T, hp, rk);
      store_schedule<NK>((uint64_t)(P.gkeys + e) + 4ull * kGcmRkWords, rk);
      store_schedule<NK>((uint64_t)(P.gkeys + (e ^ 1u)) + 4ull * kGcmRkWords, rk);
    }
    aes_expand<NK>(T, key, rk);
    const uint64_t a = (uint64_t)(P.gkeys + e);
    store_schedule<NK>(a, rk);
    gst<u32x2>(a + 8ull * kGcmRkWords, u32x2{iv[0], iv[1]});
    gst<uint32_t>(a + 8ull * kGcmRkWords + 8, iv[2]);
    uint32_t h[4] = {0u, 0u, 0u, 0u};  // H = E(K, 0^128)
    aes_block_t0<NK + 6, false>(T, [&](int r, uint32_t (&k)[4]) {
#pragma unroll
      for (int c = 0; c < 4; c++) k[c] = rk[4 * r + c];
    }, h);
    gst<u32x4>((uint64_t)(P.hkey + 4ull * e),
               u32x4{__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]),
                     __builtin_bswap32(h[3])});
  }
}

template <uint32_t SUITE>
__global__ __launch_bounds__(kKBlock) void quic_derive(const QKeysParams P) {
  constexpr bool H384 = SUITE == SQOBFS_QUIC_AES_256_GCM;
  constexpr int HL = H384 ? 48 : 32;
  __shared__ uint32_t T[256];
  if (SUITE != SQOBFS_QUIC_CHACHA20_POLY1305) stage_t0<kKBlock>(P.t0, T);
  const uint32_t i = blockIdx.x * kKBlock + threadIdx.x;
  if (i >= P.n) return;
  const uint32_t c = P.conn[i];
  const bool fresh = P.secrets != nullptr;  // wave-uniform
  uint32_t s[12], g = 0;
  if (fresh) {
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(P.secrets + (uint64_t)kQuicSecretBytes * i);
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = k < HL / 4 ? __builtin_bswap32(sp[k]) : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = P.sec[(uint64_t)kQuicSecretWords * c + k];
    g = P.gen[c];
  }
  Prf<H384> prf;
  // pass 0: the given secret (a new connection: generation 0 with hp), then
  // its "quic ku" successor; pass 1: the successor's key and iv
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    prf.set_key(s);
    if (pass == 0) {
      if (fresh) derive_entry<SUITE, true>(P, prf, T, 2 * c);
      uint32_t d[12];
      prf.template expand<kLblKu, HL>(d);
#pragma unroll
      for (int k = 0; k < 12; k++) s[k] = d[k];
      g += 1;
    } else {
      derive_entry<SUITE, false>(P, prf, T, 2 * c + (g & 1u));
    }
  }
#pragma unroll
  for (int k = 0; k < 12; k += 4)
    gst<u32x4>((uint64_t)(P.sec + (uint64_t)kQuicSecretWords * c + k),
               u32x4{s[k], s[k + 1], s[k + 2], s[k + 3]});
  P.gen[c] = g;
}

// ---------------------------------------------------------------- GHASH tables

// One wave per entry to build; lane l owns row l of the entry's 64 rows
// (hpos[0..32) then htab[0..32), contiguous in QuicGcmKeyDev).
__global__ __launch_bounds__(kTBlock) void quic_gcm_tables(const QKeysParams P) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * (kTBlock / kWave) + threadIdx.x / kWave;
  const bool fresh = P.secrets != nullptr;
  if (w >= (fresh ? 2 * P.n : P.n)) return;  // wave-uniform
  uint32_t e;
  if (fresh) {
    e = 2 * P.conn[w >> 1] + (w & 1u);
  } else {  // the entry of the newest generation (quic_derive advanced gen)
    const uint32_t c = P.conn[w];
    e = 2 * c + (P.gen[c] & 1u);
  }
  const u32x4 hv = gld<u32x4>((uint64_t)(P.hkey + 4ull * e));
  const G4 h = {{hv.x, hv.y, hv.z, hv.w}};
  G4 p;
  uint32_t swz = 0;
  if (lane < 32) {  // hpos row j: H x^(4 (31 - j))
    p = h;
    for (uint32_t k = 0; k < 4 * (31 - lane); k++) p = g_mulx(p);
  } else {  // htab row pw: (H^4)^(pw + 1), most significant exponent bit first
    const uint32_t pw = lane - 32, ex = pw + 1;
    const G4 h2 = g_mul(h, h), h4 = g_mul(h2, h2);
    p = h4;
    bool started = false;
#pragma unroll 1
    for (int b = 5; b >= 0; b--) {
      const bool bit = (ex >> b) & 1u;
      if (started) {
        p = g_mul(p, p);
        if (bit) p = g_mul(p, h4);
      } else {
        started = bit;
      }
    }
    swz = pw & 15u;
  }
  // Shoup's nibble multiples: 8 = p, 4 = p x, 2 = p x^2, 1 = p x^3
  G4 b[4];
  b[3] = p;
  b[2] = g_mulx(b[3]);
  b[1] = g_mulx(b[2]);
  b[0] = g_mulx(b[1]);
  const uint64_t row = (uint64_t)(&P.gkeys[e].hpos[0][0][0]) + 256ull * lane;
#pragma unroll
  for (uint32_t n = 0; n < 16; n++) {
    G4 v = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (n & (1u << k)) v = g_xor(v, b[k]);
    gst<u32x4>(row + 16ull * (n ^ swz), u32x4{v.w[0], v.w[1], v.w[2], v.w[3]});
  }
}
static_assert(offsetof(QuicGcmKeyDev, htab) == offsetof(QuicGcmKeyDev, hpos) + 32 * 256,
              "htab rows follow the hpos rows");
static_assert(offsetof(QuicGcmKeyDev, hpos) % 16 == 0 && sizeof(QuicGcmKeyDev) % 16 == 0 &&
                  sizeof(QuicKeyDev) % 16 == 0,
              "16-byte vector stores into keyring entries");

// ---------------------------------------------------------------- key phase

// NR 0: ChaCha20 header protection; 10 / 14: AES-ECB under the entry's hrk
// OB: the Salamander layer is still on (offsets are the packet's, after the salt)
template <int NR, bool OB>
__global__ __launch_bounds__(kPBlock) void quic_key_phase(const QPhaseParams P) {
  __shared__ uint32_t T[256];
  if (NR) stage_t0<kPBlock>(P.t0, T);
  const uint64_t i = (uint64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= P.n) return;
  const uint32_t kid = P.key_id ? P.key_id[i] : 0u;
  uint32_t out = kid;
  uint32_t len = P.in_len[i];
  const uint32_t pno = P.pn_offset[i];
  if (OB) len = len >= (uint32_t)kSalamanderSalt && len <= kQMaxPacket ? len - kSalamanderSalt : 0u;
  if (kid < P.n_keys && len >= 16 && len <= kQMaxPacket && pno + 4 + 16 <= len) {
    const uint64_t wire = (uint64_t)P.in + P.in_off[i], src = OB ? wire + kSalamanderSalt : wire;
    uint32_t first = gld<uint8_t>(src), okey[8];
    if (OB) {
      uint32_t osalt[4];
      load16(wire, wire + kSalamanderSalt, osalt);
      salamander_key(&P.opsk, osalt, okey);
      first ^= okey[0] & 0xFFu;
    }
    if (!(first & 0x80u)) {  // short header: bit 0x04 is the Key Phase
      uint32_t s[4], mask0;
      load16(src + pno + 4, src + len, s);
      if (OB) {  // key byte k covers packet byte k mod 32
        uint32_t kw[4];
        keywin(okey, pno + 4, kw);
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] ^= kw[k];
      }
      if (NR == 0) {
        uint32_t hp[8], o[16];
        const uint64_t a = (uint64_t)(P.keys + kid) + 44;
#pragma unroll
        for (int k = 0; k < 8; k++) hp[k] = gld<uint32_t>(a + 4 * k);
        const uint32_t nonce[3] = {s[1], s[2], s[3]};
        chacha20_block(hp, s[0], nonce, o);
        mask0 = o[0];
      } else {
        const uint64_t a = (uint64_t)(P.gkeys + kid) + 4ull * kGcmRkWords;
        aes_block_t0<(NR ? NR : 10), true>(T, [&](int r, uint32_t (&k)[4]) {
          const u32x4 v = gld<u32x4>(a + 16ull * r);
          k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
        }, s);
        mask0 = s[0];
      }
      out = (kid & ~1u) | (((first ^ (mask0 & 0x1Fu)) >> 2) & 1u);
    }
  }
  P.key_id_out[i] = (uint16_t)out;
}

}  // namespace sq

extern "C" int sq_launch_quic_rekey(const sq::QKeysParams *kp, void *stream) {
  using namespace sq;
  if (kp->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((kp->n + kKBlock - 1) / kKBlock);
  (void)hipGetLastError();  // (a stale error is not this launch's: sq_kernels.hip launch_k)
  if (kp->suite == SQOBFS_QUIC_CHACHA20_POLY1305) {
    hipLaunchKernelGGL((quic_derive<SQOBFS_QUIC_CHACHA20_POLY1305>), grid, dim3(kKBlock), 0, s, *kp);
  } else {
    if (kp->suite == SQOBFS_QUIC_AES_256_GCM)
      hipLaunchKernelGGL((quic_derive<SQOBFS_QUIC_AES_256_GCM>), grid, dim3(kKBlock), 0, s, *kp);
    else
      hipLaunchKernelGGL((quic_derive<SQOBFS_QUIC_AES_128_GCM>), grid, dim3(kKBlock), 0, s, *kp);
    if (hipGetLastError() != hipSuccess) return -3;
    const uint64_t waves = (uint64_t)kp->n * (kp->secrets ? 2 : 1), wpb = kTBlock / kWave;
    hipLaunchKernelGGL(quic_gcm_tables, dim3((uint32_t)((waves + wpb - 1) / wpb)), dim3(kTBlock),
                       0, s, *kp);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int sq_launch_quic_key_phase(const sq::QPhaseParams *pp, void *stream) {
  using namespace sq;
  if (pp->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((pp->n + kPBlock - 1) / kPBlock);
  (void)hipGetLastError();
  const int nr = pp->suite == SQOBFS_QUIC_CHACHA20_POLY1305 ? 0
                 : pp->suite == SQOBFS_QUIC_AES_256_GCM     ? 14
                                                            : 10;
#define SQ_PHASE(NR, OB) hipLaunchKernelGGL((quic_key_phase<NR, OB>), grid, dim3(kPBlock), 0, s, *pp)
  if (pp->obfs) {
    if (nr == 0) SQ_PHASE(0, true);
    else if (nr == 14) SQ_PHASE(14, true);
    else SQ_PHASE(10, true);
  } else {
    if (nr == 0) SQ_PHASE(0, false);
    else if (nr == 14) SQ_PHASE(14, false);
    else SQ_PHASE(10, false);
  }
#undef SQ_PHASE
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
