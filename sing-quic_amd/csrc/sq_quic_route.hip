// sq_quic_route.hip -- gfx950 routing of received QUIC datagrams to their
// connections (RFC 9000 17.2 / 17.3 headers, 12.3 packet-number spaces).
//
// Replaces, for a whole ragged receive batch, what a quic-go listener does
// per datagram on the host between the socket and the packet handlers
//   packet_handler_map.go / transport.go  handlePacket: first byte, connection
//     id lookup, long-header type, stateless-reset and unknown-id handling
//   internal/wire/header.go  ParseConnectionID, parseHeader (to the Length)
// (quic-go v0.52.0-beta.1, go.mod:7; not in the reference tree), and, under
// Hysteria2, the Salamander pass that has to come before any of it
// (hysteria2/salamander.go:42-55): on the wire even the first byte is
// obfuscated.  The datagrams are not modified: what comes out is the batch in
// the array form that sqobfs_quic_key_phase / _open / _initial_open take,
// partitioned by class, with key_id, pn_offset and pn filled in.
//
// Work decomposition, three launches per call, none of which waits on
// another workgroup (no look-back, no flags: ordering is the stream's):
//   1. quic_route<OB>: one lane per datagram, 256 per workgroup.  The lane
//      loads the packet's first 32 bytes once (load_head32; OB: derives the
//      datagram's Salamander key from the keyring's device entry and XORs
//      the head in registers), classifies the first byte, takes the
//      connection id out of the head words with v_alignbyte (byte 1 of a
//      short header, byte 6 of a long one: never past byte 26), hashes it and
//      probes the table: a 32-byte slot is two 16-byte loads, and the table
//      is at most half full, so a probe is one or two slots.  Handshake and
//      0-RTT headers go on byte by byte past byte 32 (SCID length, Length
//      varint: at most byte 54), each byte XORed with its key byte.  It reads
//      the connection's largest packet number of the class's space and
//      writes cls[i] and a 16-byte record + the number to the workspace.
//      Class counts: one ballot per class and wave, the wave's popcounts in
//      LDS, summed by eight lanes and written once per workgroup.
//   2. quic_route_scan: one workgroup, wave c scans class c's workgroup
//      counts 64 at a time (shuffle scan + running total) into exclusive
//      bases in place, then one lane writes count[8] and the class bases.
//   3. quic_route_scatter: the lane grid of (1).  A lane's rank in its class
//      = ballot prefix in the wave + the earlier waves' counts (LDS) + the
//      workgroup's base + the class base, so input order is kept within a
//      class and a wave's stores within a class are contiguous.
// The plain instantiation holds no BLAKE2b state: its registers are the head
// words and the header cursor.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/sqobfs.h"
#include "sq_bytes.h"
#include "sq_hash.h"
#include "sq_internal.h"
#include "sq_obfs_key.h"
#include "sq_quic.h"

namespace sq {

constexpr uint32_t kRWaves = kRouteBlock / kWave;
constexpr uint32_t kScanBlock = 8 * kWave;  // a wave per class
constexpr uint32_t kNoClass = 7;            // a lane past the batch
constexpr uint32_t kPnInitial = 0, kPnHandshake = 1, kPnApp = 2;  // pn_state columns

// the connection of the zero-padded connection id d, or kQuicNoConn
__device__ __forceinline__ uint32_t cid_lookup(const QRouteParams &P,
                                               const uint32_t (&d)[kCidWords]) {
  uint32_t s = cid_hash(d) & P.slot_mask;
  // (ends at the first empty slot: the table is at most half full; the bound
  // only keeps a damaged table from holding the lane)
  for (uint32_t k = 0; k <= P.slot_mask; k++) {
    const uint64_t a = (uint64_t)(P.slots + s);
    const u32x4 x = gld<u32x4>(a), y = gld<u32x4>(a + 16);
    if (y.y == kQuicNoConn) break;
    if (((x.x ^ d[0]) | (x.y ^ d[1]) | (x.z ^ d[2]) | (x.w ^ d[3]) | (y.x ^ d[4])) == 0)
      return y.y;
    s = (s + 1) & P.slot_mask;
  }
  return kQuicNoConn;
}

// cid_len bytes at byte O of the head (O + 20 <= 28), zero-padded
template <uint32_t O>
__device__ __forceinline__ void head_cid(const uint32_t (&hd)[8], uint32_t cid_len,
                                         uint32_t (&d)[kCidWords]) {
#pragma unroll
  for (int j = 0; j < (int)kCidWords; j++)
    d[j] = __builtin_amdgcn_alignbyte(hd[j + O / 4 + 1], hd[j + O / 4], O & 3) &
           range_mask(0, (int)cid_len, j);
}

// The class of the datagram of dlen bytes at wire, and what the class's
// consumer needs: conn, pno (the packet-number offset), len_out (in_len of
// the partitioned batch) and the packet-number space whose largest number
// decodes it.
template <bool OB>
__device__ __forceinline__ uint32_t classify(const QRouteParams &P, uint64_t wire, uint32_t dlen,
                                             uint32_t &conn, uint32_t &pno, uint32_t &len_out,
                                             uint32_t &space) {
  conn = kQuicNoConn;
  pno = 0;
  len_out = dlen;
  space = kPnApp;
  uint64_t src = wire;
  uint32_t len = dlen, hd[8], okey[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (OB) {  // salt8 || packet ^ K: at least one packet byte
    if (dlen <= (uint32_t)kSalamanderSalt) return SQOBFS_QUIC_ROUTE_MALFORMED;
    uint32_t osalt[4];
    load16(wire, wire + kSalamanderSalt, osalt);
    salamander_key(P.opsk, osalt, okey);
    src += kSalamanderSalt;
    len -= kSalamanderSalt;
  } else if (len == 0) {
    return SQOBFS_QUIC_ROUTE_MALFORMED;
  }
  load_head32(src, len, hd);
  if (OB) {  // key byte k covers packet byte k mod 32
#pragma unroll
    for (int j = 0; j < 8; j++) hd[j] ^= okey[j] & range_mask(0, (int)(len < 32 ? len : 32), j);
  }
  auto hb = [&](uint32_t k) -> uint32_t {
    const uint32_t b = head_byte(hd, src, k);
    return (OB && k >= 32) ? b ^ byte32(okey, k & 31) : b;
  };
  const uint32_t first = hd[0] & 0xFFu;
  uint32_t d[kCidWords];
  if (!(first & 0x80u)) {  // short header (RFC 9000 17.3.1): first || DCID || pn
    if (!(first & 0x40u) || len < 1 + P.cid_len) return SQOBFS_QUIC_ROUTE_MALFORMED;
    head_cid<1>(hd, P.cid_len, d);
    conn = cid_lookup(P, d);
    if (conn == kQuicNoConn) return SQOBFS_QUIC_ROUTE_UNKNOWN;
    pno = 1 + P.cid_len;
    return SQOBFS_QUIC_ROUTE_SHORT;
  }
  // long header (17.2): first || version || dcid_len || DCID || scid_len || SCID ...
  if (len < 5) return SQOBFS_QUIC_ROUTE_MALFORMED;
  if (__builtin_bswap32(__builtin_amdgcn_alignbyte(hd[1], hd[0], 1)) != 1u)
    return SQOBFS_QUIC_ROUTE_OTHER;
  if (!(first & 0x40u)) return SQOBFS_QUIC_ROUTE_MALFORMED;
  const uint32_t type = (first >> 4) & 3u;
  if (type == 3) return SQOBFS_QUIC_ROUTE_OTHER;  // Retry: no packet number, no keys here
  const uint32_t dl = (hd[1] >> 8) & 0xFFu;       // byte 5 (zero when len is 5)
  if (dl > kCidWords * 4 || 6 + dl > len) return SQOBFS_QUIC_ROUTE_MALFORMED;
  head_cid<6>(hd, P.cid_len, d);
  if (type == 0) {  // Initial: keyed by its own DCID, a connection only for later ones
    if (dl == P.cid_len) conn = cid_lookup(P, d);
    space = kPnInitial;
    return SQOBFS_QUIC_ROUTE_INITIAL;
  }
  // Handshake (10) / 0-RTT (01): scid_len || SCID || Length (varint) || pn
  if (6 + dl >= len) return SQOBFS_QUIC_ROUTE_MALFORMED;
  const uint32_t sl = byte32(hd, 6 + dl);  // (at most byte 26)
  uint32_t p = 7 + dl + sl;
  if (sl > kCidWords * 4 || p >= len) return SQOBFS_QUIC_ROUTE_MALFORMED;
  const uint32_t b0 = hb(p), nb = 1u << (b0 >> 6);  // RFC 9000 16
  if (p + nb > len) return SQOBFS_QUIC_ROUTE_MALFORMED;
  uint64_t length = b0 & 0x3Fu;
  for (uint32_t k = 1; k < nb; k++) length = (length << 8) | hb(p + k);
  p += nb;
  if (length > len - p) return SQOBFS_QUIC_ROUTE_MALFORMED;  // (p <= len)
  if (dl != P.cid_len) return SQOBFS_QUIC_ROUTE_UNKNOWN;
  conn = cid_lookup(P, d);
  if (conn == kQuicNoConn) return SQOBFS_QUIC_ROUTE_UNKNOWN;
  pno = p;
  len_out = p + (uint32_t)length + (OB ? (uint32_t)kSalamanderSalt : 0u);
  space = type == 2 ? kPnHandshake : kPnApp;
  return type == 2 ? SQOBFS_QUIC_ROUTE_HANDSHAKE : SQOBFS_QUIC_ROUTE_ZERO_RTT;
}

// The lane's rank among the lanes of its class in its wave; lane 0 leaves
// the wave's count of every class in wcnt.  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t class_rank(uint32_t cls, uint32_t lane, uint32_t (&wcnt)[8]) {
  uint32_t rank = 0;
#pragma unroll
  for (uint32_t c = 0; c < 8; c++) {
    const uint64_t m = __ballot(cls == c);
    if (cls == c) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[c] = (uint32_t)__popcll(m);
  }
  return rank;
}

template <bool OB>
__global__ __launch_bounds__(kRouteBlock) void quic_route(const QRouteParams P) {
  __shared__ uint32_t wcnt[kRWaves][8];
  const uint64_t i = (uint64_t)blockIdx.x * kRouteBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  uint32_t cls = kNoClass;
  if (i < P.n) {
    uint32_t conn, pno, len_out, space;
    cls = classify<OB>(P, (uint64_t)P.in + P.in_off[i], P.in_len[i], conn, pno, len_out, space);
    const uint64_t pn =  // (a connection comes from the table: below conns)
        conn != kQuicNoConn ? gld<uint64_t>((uint64_t)(P.pn_state + 3ull * conn + space)) : 0ull;
    P.r_cls[i] = (uint8_t)cls;
    gst<u32x4>((uint64_t)(P.ws_rec + 4 * i), u32x4{conn, len_out, pno | (cls << 16), 0u});
    P.ws_pn[i] = pn;
  }
  class_rank(cls, lane, wcnt[wv]);
  __syncthreads();
  if (threadIdx.x < 8) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kRWaves; w++) sum += wcnt[w][threadIdx.x];
    P.ws_wg[8ull * blockIdx.x + threadIdx.x] = threadIdx.x < kRouteClasses ? sum : 0u;
  }
}

// ws_wg[g][c]: the count of class c in workgroup g -> the count in the
// workgroups before g; ws_base[c]: the datagrams of the classes before c.
__global__ __launch_bounds__(kScanBlock) void quic_route_scan(const QRouteParams P) {
  __shared__ uint32_t tot[8];
  const uint32_t lane = threadIdx.x & (kWave - 1), c = threadIdx.x / kWave;
  uint32_t run = 0;
  for (uint32_t g0 = 0; g0 < P.nwg; g0 += kWave) {
    const uint32_t g = g0 + lane;
    const uint32_t v = g < P.nwg ? P.ws_wg[8ull * g + c] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (g < P.nwg) P.ws_wg[8ull * g + c] = run + inc - v;
    run += __shfl(inc, kWave - 1);
  }
  if (lane == 0) tot[c] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0;
    for (uint32_t k = 0; k < 8; k++) {
      P.ws_base[k] = b;
      P.r_count[k] = tot[k];
      b += tot[k];
    }
  }
}

__global__ __launch_bounds__(kRouteBlock) void quic_route_scatter(const QRouteParams P) {
  __shared__ uint32_t wcnt[kRWaves][8];
  const uint64_t i = (uint64_t)blockIdx.x * kRouteBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  u32x4 r = {0u, 0u, kNoClass << 16, 0u};
  if (i < P.n) r = gld<u32x4>((uint64_t)(P.ws_rec + 4 * i));
  const uint32_t cls = r.z >> 16;
  uint32_t dst = class_rank(cls, lane, wcnt[wv]);
  __syncthreads();
  if (i >= P.n) return;
#pragma unroll
  for (uint32_t w = 0; w + 1 < kRWaves; w++) dst += w < wv ? wcnt[w][cls] : 0u;
  dst += P.ws_base[cls] + P.ws_wg[8ull * blockIdx.x + cls];  // (< n: a rank among n datagrams)
  const bool keyed = cls == SQOBFS_QUIC_ROUTE_SHORT || cls == SQOBFS_QUIC_ROUTE_HANDSHAKE ||
                     cls == SQOBFS_QUIC_ROUTE_ZERO_RTT;
  P.r_order[dst] = (uint32_t)i;
  P.r_in_off[dst] = P.in_off[i];
  P.r_in_len[dst] = r.y;
  if (P.r_out_off) P.r_out_off[dst] = P.out_off[i];
  P.r_pn_offset[dst] = (uint16_t)r.z;
  P.r_pn[dst] = P.ws_pn[i];
  P.r_key_id[dst] = keyed ? (uint16_t)(2 * r.x) : (uint16_t)0;
  P.r_conn[dst] = r.x;
}

constexpr uint32_t kPnBlock = 256;

__global__ __launch_bounds__(kPnBlock) void quic_pn_commit(uint64_t *pn_state, uint32_t conns,
                                                          uint32_t space, uint32_t n,
                                                          const uint32_t *conn,
                                                          const uint32_t *out_len,
                                                          const uint64_t *pn_out) {
  const uint64_t j = (uint64_t)blockIdx.x * kPnBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t c = conn[j];
  // (kQuicNoConn is above every conns; the codes are the top four values)
  if (c >= conns || out_len[j] >= SQOBFS_QUIC_EHEADER) return;
  // several packets of one connection sit in a batch: a 64-bit vector atomic
  atomicMax((unsigned long long *)(pn_state + 3ull * c + space), (unsigned long long)pn_out[j]);
}

__global__ __launch_bounds__(kPnBlock) void quic_pn_reset(uint64_t *pn_state, uint32_t conns,
                                                         uint32_t n, const uint32_t *conn) {
  const uint64_t j = (uint64_t)blockIdx.x * kPnBlock + threadIdx.x;
  if (j >= 3ull * n) return;
  const uint32_t c = conn[j / 3];
  if (c < conns) pn_state[3ull * c + j % 3] = 0;
}

}  // namespace sq

extern "C" int sq_launch_quic_route(const sq::QRouteParams *rp, void *stream) {
  using namespace sq;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();  // (a stale error is not this launch's: sq_kernels.hip launch_k)
  if (rp->n) {
    if (rp->obfs) hipLaunchKernelGGL((quic_route<true>), dim3(rp->nwg), dim3(kRouteBlock), 0, s, *rp);
    else hipLaunchKernelGGL((quic_route<false>), dim3(rp->nwg), dim3(kRouteBlock), 0, s, *rp);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  hipLaunchKernelGGL(quic_route_scan, dim3(1), dim3(kScanBlock), 0, s, *rp);  // n == 0: count = 0
  if (hipGetLastError() != hipSuccess) return -3;
  if (rp->n) hipLaunchKernelGGL(quic_route_scatter, dim3(rp->nwg), dim3(kRouteBlock), 0, s, *rp);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int sq_launch_quic_pn_commit(uint64_t *pn_state, uint32_t conns, uint32_t space,
                                        uint32_t n, const uint32_t *conn, const uint32_t *out_len,
                                        const uint64_t *pn_out, void *stream) {
  using namespace sq;
  if (n == 0) return 0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(quic_pn_commit, dim3((uint32_t)(((uint64_t)n + kPnBlock - 1) / kPnBlock)),
                     dim3(kPnBlock), 0, (hipStream_t)stream, pn_state, conns, space, n, conn,
                     out_len, pn_out);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int sq_launch_quic_pn_reset(uint64_t *pn_state, uint32_t conns, uint32_t n,
                                       const uint32_t *conn, void *stream) {
  using namespace sq;
  if (n == 0) return 0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(quic_pn_reset, dim3((uint32_t)((3ull * n + kPnBlock - 1) / kPnBlock)),
                     dim3(kPnBlock), 0, (hipStream_t)stream, pn_state, conns, n, conn);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
