// k_keccak.hip -- Keccak-256 as Ethereum uses it (the original padding 0x01 ... 0x80, not SHA-3's 0x06), one message per lane, and the two kernels that make
// an address of a public key and a recovery id of Ethereum's v.
//
//   * k_keccak256<ALIGN, PER_LANE>   the sponge over message i at msg + i * stride: whole blocks in THE loop of this file (8-, 4- or 1-byte loads as the base
//                                    and the stride allow), the last block and the padding behind it (keccak.cuh: keccak_absorb_last, no branch).  PER_LANE:
//                                    lane i absorbs min(lens[i], stride) bytes and the loop's trip count is the lane's own; else every lane absorbs msg_bytes
//                                    and the loop is uniform.  The digest leaves as sha256's does: 4 x u64 little-endian limbs of the big-endian integer.
//   * k_eth_address<HAS_OK>          one permutation per lane: the block is be32(qx) || be32(qy), the pad byte and the final bit are constants of lanes 8
//                                    and 16; bytes 12 .. 31 of the digest go to addr + 20 i, zeros where ok[i] = 0.
//   * k_eth_recovery_id              v in {0, 1, 27, 28} -> 0, 1, 0, 1; anything else, and s > n / 2 where EIP-2's rule is asked for, -> 0xff: the lift
//                                    of k_recover.hip refuses every v above 3, so the lane comes out of the recovery's own kernels with ok = 0 and a zero key.
//
// PUBLIC data throughout: messages, public keys, signatures.  None of these kernels takes a secret, and their loads and the loop depend on the data's length.
// The only conditional branches are each kernel's bounds exit and k_keccak256's block loop (tests/test_keccak_cpu.py reads the listing).
#include "kernels.h"
#include "keccak.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

KECCAK_DEV uint32_t lo32(uint64_t x) { return (uint32_t)x; }
KECCAK_DEV uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
KECCAK_DEV uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

template <int ALIGN, bool PER_LANE>
__global__ void __launch_bounds__(BLOCK) k_keccak256(const uint8_t* msg, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens, uint64_t* out, size_t n) {
  GID;
  size_t len = msg_bytes;
  if constexpr (PER_LANE) { len = lens[i]; len = len < stride ? len : stride; }                   // never past the lane's own stride
  const uint8_t* p = msg + i * stride;
  uint4* o = reinterpret_cast<uint4*>(out + 4 * i);
  keccak_state s = keccak_zero();
  const size_t full = len / KECCAK_RATE;
#pragma unroll 1
  for (size_t b = 0; b < full; ++b) {                                                             // the block loop
    keccak_absorb_block<ALIGN>(s, p);
    keccak_f1600(s);
    p += KECCAK_RATE;
  }
  keccak_absorb_last<ALIGN>(s, p, (uint32_t)(len - full * KECCAK_RATE), 0x01u, reinterpret_cast<const uint8_t*>(o));
  keccak_f1600(s);
  // digest byte k is byte k of the first four lanes; the integer's most significant limb is lane 0 with its bytes reversed
  o[0] = make_uint4(bswap(hi32(s.a[3])), bswap(lo32(s.a[3])), bswap(hi32(s.a[2])), bswap(lo32(s.a[2])));
  o[1] = make_uint4(bswap(hi32(s.a[1])), bswap(lo32(s.a[1])), bswap(hi32(s.a[0])), bswap(lo32(s.a[0])));
}

// lanes 0 .. 3 = the limbs of qx from the top, bytes reversed; 4 .. 7 the same of qy; byte 64 = 0x01, byte 135 = 0x80
template <bool HAS_OK>
__global__ void __launch_bounds__(BLOCK) k_eth_address(const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, const uint8_t* __restrict__ okv,
                                                       uint32_t* __restrict__ addr, size_t n) {
  GID;
  const uint4* x = reinterpret_cast<const uint4*>(qx + 4 * i);
  const uint4* y = reinterpret_cast<const uint4*>(qy + 4 * i);
  const uint4 x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
  auto lane = [](uint32_t w_lo, uint32_t w_hi) { return ((uint64_t)bswap(w_lo) << 32) | bswap(w_hi); };      // one limb (its two words) as Keccak reads its big-endian bytes
  keccak_state s = keccak_zero();
  s.a[0] = lane(x1.z, x1.w); s.a[1] = lane(x1.x, x1.y); s.a[2] = lane(x0.z, x0.w); s.a[3] = lane(x0.x, x0.y);
  s.a[4] = lane(y1.z, y1.w); s.a[5] = lane(y1.x, y1.y); s.a[6] = lane(y0.z, y0.w); s.a[7] = lane(y0.x, y0.y);
  s.a[8] = 0x01ull;
  s.a[16] = 0x8000000000000000ull;
  keccak_f1600(s);
  uint32_t keep = 0xffffffffu;
  if constexpr (HAS_OK) keep = 0u - (uint32_t)(okv[i] != 0);
  uint32_t* a = addr + 5 * i;                                                                     // digest bytes 12 .. 31, in order (little-endian stores)
  a[0] = hi32(s.a[1]) & keep; a[1] = lo32(s.a[2]) & keep; a[2] = hi32(s.a[2]) & keep; a[3] = lo32(s.a[3]) & keep; a[4] = hi32(s.a[3]) & keep;
}

// half = n / 2 (integer halving); low_s: 0 or 1, the same for every lane
__global__ void __launch_bounds__(BLOCK) k_eth_recovery_id(words8 half, const uint8_t* __restrict__ vv, const uint64_t* __restrict__ sv, uint8_t* __restrict__ out, size_t n,
                                                           uint32_t low_s) {
  GID;
  const uint4* sp = reinterpret_cast<const uint4*>(sv + 4 * i);
  const uint4 s0 = sp[0], s1 = sp[1];
  const uint32_t s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  uint32_t borrow = 0;                                                                            // of half - s: 1 where s > n / 2
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t d = (uint64_t)half.w[k] - s[k] - borrow;
    borrow = (uint32_t)(d >> 32) & 1u;
  }
  const uint32_t v = vv[i];
  const uint32_t id = v >= 27u ? v - 27u : v;                                                     // 27, 28 -> 0, 1; 2 and 3 stay what they are (28 + ... stays above 1)
  const uint32_t refused = (uint32_t)(id > 1u) | (borrow & low_s);
  out[i] = (uint8_t)(refused ? 0xffu : id);
}

template <int ALIGN> void launch_keccak(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride, const uint32_t* lens, uint64_t* e, size_t n) {
  if (lens) hipLaunchKernelGGL((k_keccak256<ALIGN, true>), launch::grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride, lens, e, n);
  else hipLaunchKernelGGL((k_keccak256<ALIGN, false>), launch::grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride, lens, e, n);
}
}  // namespace

namespace launch {
void keccak256(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(msg) | stride_bytes;
  if ((bits & 7u) == 0) launch_keccak<8>(s, msg, msg_bytes, stride_bytes, lens, e, n);
  else if ((bits & 3u) == 0) launch_keccak<4>(s, msg, msg_bytes, stride_bytes, lens, e, n);
  else launch_keccak<1>(s, msg, msg_bytes, stride_bytes, lens, e, n);
}
void eth_address(hipStream_t s, const uint64_t* qx, const uint64_t* qy, const uint8_t* ok, uint8_t* addr, size_t n) {
  uint32_t* a = reinterpret_cast<uint32_t*>(addr);
  if (ok) hipLaunchKernelGGL(k_eth_address<true>, grid_for(n), dim3(BLOCK), 0, s, qx, qy, ok, a, n);
  else hipLaunchKernelGGL(k_eth_address<false>, grid_for(n), dim3(BLOCK), 0, s, qx, qy, ok, a, n);
}
void eth_recovery_id(hipStream_t s, const words8& half, const uint8_t* v, const uint64_t* sg, uint8_t* out, size_t n, bool low_s) {
  hipLaunchKernelGGL(k_eth_recovery_id, grid_for(n), dim3(BLOCK), 0, s, half, v, sg, out, n, low_s ? 1u : 0u);
}
}  // namespace launch
}  // namespace ecsimd_hip
