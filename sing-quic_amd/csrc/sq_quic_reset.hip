// sq_quic_reset.hip -- gfx950 QUIC stateless resets (RFC 9000 10.3): building
// them for datagrams this endpoint can no longer place, and recognising the
// peer's in datagrams that nothing else accounts for.
//
// Replaces, for a whole ragged batch per launch, what a quic-go listener does
// per stray datagram on the host
//   transport.go  maybeSendStatelessReset / sendStatelessReset
//   internal/handshake  (stateless_reset.go) GetStatelessResetToken
//   packet_handler_map.go / transport.go  handlePacket: the last 16 bytes of a
//     short-header datagram against the tokens its connections were given
// (quic-go v0.52.0-beta.1, go.mod:7; not in the reference tree), and under
// Hysteria2 the Salamander pass on both sides of it: the trigger arrives
// obfuscated, the reset leaves obfuscated, and a received reset's last 16
// bytes are key bytes until the layer is taken off.
//
// Both kernels: one lane per datagram, 256 per workgroup, no loop over the
// grid (nothing is staged per workgroup that a persistent grid would save).
//
// quic_reset<OB>, the lane's work:
//   head     load_head32 (the trigger's first 32 bytes, never past in_len);
//            OB: the datagram's Salamander key, XORed over the head
//   token    HMAC-SHA256(key, cid)[0..16) in exactly two compressions: the
//            key's pad midstates come wave-uniform from the kernarg segment,
//            the inner block is the id taken out of the head words one byte
//            in (v_alignbyte), masked at cid_len, with the 0x80 pad merged in
//            and the words byte-swapped; the outer block is the inner digest
//   filler   one ChaCha20 block per lane, counter = the datagram's index (the
//            plain form; see DESIGN.md 9.4.6 for why not the quad form)
//   row      LDS, 112 bytes per lane:
//              [0, 96)   the datagram as it leaves: (OB: salt8 ||) filler,
//                        written as aligned 16-byte stores from registers,
//                        then the token over it at its ragged byte position
//                        R - 16 with byte-aligned stores.  OB: filler and
//                        token are XORed with the reset's own key in
//                        registers first (key word j & 7 on filler word j,
//                        the window at R - 16 on the token), so the row is
//                        written once and never read back by its lane
//              [96, 112) the output record: destination, length
//            112 = 7 x 16: the rows of consecutive lanes start 28 banks
//            apart, and 7 is odd, so the eight lanes of a 16-byte access hit
//            eight different bank quads (96 = 6 x 16 would put lanes l and
//            l + 4 on the same quad of 32 banks).
//   output   the wave copies its 64 datagrams out of the rows, eight lanes
//            per datagram, 16 bytes per lane: the datagram starts at row byte
//            0, so a lane moves one aligned LDS block to one byte-aligned
//            global store, with no funnel shift.
// quic_reset_match<OB>, the lane's work: the first byte and the last 16 bytes
// (OB: XORed with key byte 0 / the key window at (L - 16) & 31), the seeded
// hash, and a probe of span + 1 consecutive slots: one 16-byte load of a
// slot's token, all four words compared at once, and a 4-byte load of its
// connection only on equality.  The probe does not stop at an empty slot (a
// slot's token cannot say that it is empty: every 16-byte value is a valid
// token); its length is the table's longest displacement, kept by the host,
// so the trip count is wave-uniform.  hits: one ballot and one vector
// atomicAdd per wave that has a match.
// The plain instantiations hold no BLAKE2b state.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/sqobfs.h"
#include "sq_bytes.h"
#include "sq_hash.h"
#include "sq_internal.h"
#include "sq_obfs_key.h"
#include "sq_quic.h"

namespace sq {

constexpr uint32_t kSRow = 96, kSRowStride = 112;
static_assert(kSalamanderSalt + SQOBFS_QUIC_RESET_MAX <= kSRow, "row");
static_assert((kSRowStride / 16) % 2 == 1, "an odd number of bank quads between rows");
static_assert(kResetBlock * kSRowStride <= 64 * 1024, "LDS");

#define SQ_LDS __attribute__((address_space(3)))
typedef SQ_LDS char *lrow;
typedef uint32_t u32_a1 __attribute__((aligned(1)));
__device__ __forceinline__ void lst32(lrow p, uint32_t v) { *(SQ_LDS u32_a1 *)p = v; }
__device__ __forceinline__ void lst128(lrow p, u32x4 v) { *(SQ_LDS u32x4 *)p = v; }  // 16-aligned
__device__ __forceinline__ void lld128(lrow p, uint32_t (&w)[4]) {
  const u32x4 v = *(const SQ_LDS u32x4 *)p;
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// The datagram's packet: src and len move past the salt, ok = its key.
// Datagrams without min_len packet bytes come back with len = 0, no key made.
__device__ __forceinline__ void strip_salamander(const PskEntry *opsk, uint32_t min_len,
                                                 uint64_t &src, uint32_t &len, uint32_t (&ok)[8]) {
  if (len >= (uint32_t)kSalamanderSalt + min_len) {
    uint32_t osalt[4];
    load16(src, src + kSalamanderSalt, osalt);
    salamander_key(opsk, osalt, ok);
    src += kSalamanderSalt;
    len -= kSalamanderSalt;
  } else {
    len = 0;
  }
}

// Datagram i of the batch: its reset in the lane's row, the record behind it.
template <bool OB>
__device__ __forceinline__ void reset_lane(const QResetParams &P, uint32_t i, lrow row) {
  uint64_t src = (uint64_t)P.in + P.in_off[i];
  uint32_t len = P.in_len[i];
  uint32_t ok[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (OB) strip_salamander(P.opsk, 1, src, len, ok);
  if (len == 0) {
    P.out_len[i] = kQEShort;
    return;
  }
  uint32_t hd[8];
  load_head32(src, len, hd);
  if (OB) {
#pragma unroll
    for (int j = 0; j < 8; j++) hd[j] ^= ok[j] & range_mask(0, (int)(len < 32 ? len : 32), j);
  }
  if ((hd[0] & 0xC0u) != 0x40u) {  // long header, or the fixed bit clear
    P.out_len[i] = kQEHeader;
    return;
  }
  if (len < SQOBFS_QUIC_RESET_MIN + 1) {  // a reset is smaller than its trigger
    P.out_len[i] = kQEShort;
    return;
  }
  const uint32_t R = P.reset_len < len - 1 ? P.reset_len : len - 1;

  // token16 = HMAC-SHA256(key, packet[1 .. 1 + cid_len))[0..16)
  const uint32_t cl = P.cid_len;
  uint32_t m[16], st[8];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    uint32_t w = j < 5 ? __builtin_amdgcn_alignbyte(hd[j + 1], hd[j], 1) & range_mask(0, (int)cl, j)
                       : 0u;
    w |= (uint32_t)j == (cl >> 2) ? 0x80u << (8 * (cl & 3)) : 0u;  // (uniform)
    m[j] = __builtin_bswap32(w);
  }
#pragma unroll
  for (int j = 6; j < 15; j++) m[j] = 0u;
  m[15] = (64u + cl) * 8u;
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = P.im[j];
  s2_compress(st, m);
#pragma unroll
  for (int j = 0; j < 8; j++) m[j] = st[j];
  m[8] = 0x80000000u;
#pragma unroll
  for (int j = 9; j < 15; j++) m[j] = 0u;
  m[15] = (64u + 32u) * 8u;
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = P.om[j];
  s2_compress(st, m);
  uint32_t tk[4];
#pragma unroll
  for (int w = 0; w < 4; w++) tk[w] = __builtin_bswap32(st[w]);

  // filler = ChaCha20 block i; byte 0: a short header with the fixed bit
  uint32_t f[16];
  chacha20_block(P.fkey, i, P.fnonce, f);
  f[0] = (f[0] & 0xFFFFFF00u) | (f[0] & 0x3Fu) | 0x40u;

  uint64_t dst = (uint64_t)P.out + P.out_off[i];
  const uint32_t S = OB ? (uint32_t)kSalamanderSalt : 0u;
  if (OB) {
    // the reset's own key, from salt[i]: packet byte b gets key byte b & 31
    const u32x2 sv = gld<u32x2>((uint64_t)P.salt + 8ull * i);
    const uint32_t s4[4] = {sv.x, sv.y, 0u, 0u};
    uint32_t k2[8], kw[4];
    salamander_key(P.opsk, s4, k2);
#pragma unroll
    for (int j = 0; j < 16; j++) f[j] ^= k2[j & 7];
    keywin(k2, R - 16, kw);
#pragma unroll
    for (int w = 0; w < 4; w++) tk[w] ^= kw[w];
    lst128(row, u32x4{sv.x, sv.y, f[0], f[1]});
#pragma unroll
    for (int q = 0; q < 3; q++)
      lst128(row + 16 + 16 * q, u32x4{f[4 * q + 2], f[4 * q + 3], f[4 * q + 4], f[4 * q + 5]});
    lst128(row + 64, u32x4{f[14], f[15], 0u, 0u});
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      lst128(row + 16 * q, u32x4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]});
  }
  // (after the filler, over it: LDS keeps a lane's stores in order; ends at
  // byte S + R <= 88)
#pragma unroll
  for (int w = 0; w < 4; w++) lst32(row + S + R - 16 + 4 * w, tk[w]);
  lst128(row + kSRow, u32x4{(uint32_t)dst, (uint32_t)(dst >> 32), 0u, S + R});
  P.out_len[i] = S + R;
}

template <bool OB>
__global__ __launch_bounds__(kResetBlock) void quic_reset(const QResetParams P) {
  __shared__ __attribute__((aligned(16))) char lds[kResetBlock * kSRowStride];
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const lrow rows = (lrow)lds + wv * kWave * kSRowStride;
  const lrow row = rows + lane * kSRowStride;
  const uint64_t i = (uint64_t)blockIdx.x * kResetBlock + threadIdx.x;
  lst128(row + kSRow, u32x4{0u, 0u, 0u, 0u});  // nothing to copy
  if (i < P.n) reset_lane<OB>(P, (uint32_t)i, row);
  // the wave's datagrams leave the rows: 8 lanes per datagram, 16 bytes each
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t t = lane; t < 8 * kWave; t += kWave) {
    const lrow pr = rows + (t >> 3) * kSRowStride;
    uint32_t r[4], v[4];
    lld128(pr + kSRow, r);
    const uint32_t o = 16 * (t & 7), plen = r[3];
    if (o >= plen) continue;  // (plen <= 88: block o / 16 <= 5 is read)
    lld128(pr + o, v);
    const uint64_t D = (((uint64_t)r[1] << 32) | r[0]) + o;
    if (plen - o >= 16) gst<u32x4_a1>(D, u32x4_a1{v[0], v[1], v[2], v[3]});
    else store16(D, v, plen - o);
  }
}

template <bool OB>
__global__ __launch_bounds__(kResetBlock) void quic_reset_match(const QResetParams P) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t i = (uint64_t)blockIdx.x * kResetBlock + threadIdx.x;
  uint32_t conn = kQuicNoConn;
  if (i < P.n) {
    uint64_t src = (uint64_t)P.in + P.in_off[i];
    uint32_t len = P.in_len[i];
    uint32_t ok[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (OB) strip_salamander(P.opsk, SQOBFS_QUIC_RESET_MIN, src, len, ok);
    if (len >= SQOBFS_QUIC_RESET_MIN && P.slots) {
      uint32_t first = gld<uint8_t>(src);
      uint32_t t[kResetWords];
      load16(src + len - 16, src + len, t);
      if (OB) {
        uint32_t kw[4];
        keywin(ok, (len - 16) & 31, kw);
#pragma unroll
        for (int w = 0; w < 4; w++) t[w] ^= kw[w];
        first ^= ok[0] & 0xFFu;
      }
      if (!(first & 0x80u)) {
        uint32_t s = reset_hash(t, P.seed) & P.slot_mask;
        for (uint32_t k = 0; k <= P.span; k++) {
          const uint64_t a = (uint64_t)(P.slots + s);
          const u32x4 x = gld<u32x4>(a);
          if (((x.x ^ t[0]) | (x.y ^ t[1]) | (x.z ^ t[2]) | (x.w ^ t[3])) == 0) {
            const uint32_t c = gld<uint32_t>(a + 16);  // (an empty slot holds kQuicNoConn)
            if (c != kQuicNoConn) conn = c;
          }
          s = (s + 1) & P.slot_mask;
        }
      }
    }
    P.conn_out[i] = conn;
  }
  const uint64_t hit = __ballot(conn != kQuicNoConn);
  if (P.hits && hit && lane == (uint32_t)(__ffsll((unsigned long long)hit) - 1))
    atomicAdd(P.hits, (uint32_t)__popcll(hit));
}

}  // namespace sq

extern "C" int sq_launch_quic_reset(int match, int obfs, const sq::QResetParams *rp,
                                    void *stream) {
  using namespace sq;
  if (rp->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();  // (a stale error is not this launch's: sq_kernels.hip launch_k)
  const dim3 grid((uint32_t)(((uint64_t)rp->n + kResetBlock - 1) / kResetBlock)), block(kResetBlock);
  if (match) {
    if (obfs) hipLaunchKernelGGL((quic_reset_match<true>), grid, block, 0, s, *rp);
    else hipLaunchKernelGGL((quic_reset_match<false>), grid, block, 0, s, *rp);
  } else {
    if (obfs) hipLaunchKernelGGL((quic_reset<true>), grid, block, 0, s, *rp);
    else hipLaunchKernelGGL((quic_reset<false>), grid, block, 0, s, *rp);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
