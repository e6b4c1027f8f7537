// k_sha512.hip -- SHA-512 and HMAC-SHA-512 (RFC 2104) over a batch of equal-length messages.  PUBLIC data: lengths, strides and alignment are the same on
// every lane, every branch is uniform.
//
//   * k_sha512<ALIGNED>   one message per lane through sha512.cuh's absorb function; the 64 digest bytes go to out64 + 64 i, in order, as four 16-byte stores.
//   * k_hmac_sha512<MSG_ALIGNED, KEY_ALIGNED>  the key (at most 128 bytes: zero-padded to one block; longer: hashed first) is compressed once into its ipad and its opad
//                         midstate, the message is absorbed behind the inner one, and ONE outer tail block finishes.  key_stride == 0: one key for the call.
#include "kernels.h"
#include "sha512.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// the digest's bytes in order: every word leaves with its bytes swapped (out is 16-byte aligned)
ECS_DEV void sha512_store(uint4* __restrict__ out, size_t i, const sha512_state& s) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    out[4 * i + j] = make_uint4(__builtin_bswap32((uint32_t)(s.h[2 * j] >> 32)), __builtin_bswap32((uint32_t)s.h[2 * j]),
                                __builtin_bswap32((uint32_t)(s.h[2 * j + 1] >> 32)), __builtin_bswap32((uint32_t)s.h[2 * j + 1]));
}

template <bool ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_sha512(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint4* __restrict__ out, size_t n) {
  GID;
  sha512_state s = sha512_iv();
  sha512_absorb_message<ALIGNED>(s, msg + i * stride, msg_bytes, 0);
  sha512_store(out, i, s);
}

// MSG_ALIGNED / KEY_ALIGNED: base and stride of the messages / of the keys are multiples of 4 (a key of at most 128 bytes is read by bytes either way)
template <bool MSG_ALIGNED, bool KEY_ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_hmac_sha512(const uint8_t* __restrict__ key, size_t key_bytes, size_t key_stride, const uint8_t* __restrict__ msg, size_t msg_bytes,
                                                       size_t stride, uint4* __restrict__ out, size_t n) {
  GID;
  const uint8_t* kp = key + i * key_stride;
  sha512_block kb;
  if (key_bytes > 128) {
    sha512_state ks = sha512_iv();
    sha512_absorb_message<KEY_ALIGNED>(ks, kp, key_bytes, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) { kb.w[j] = ks.h[j]; kb.w[8 + j] = 0u; }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint64_t w = 0;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        uint64_t byte = 0;
        if ((size_t)(8 * j + t) < key_bytes) byte = kp[8 * j + t];
        w = (w << 8) | byte;
      }
      kb.w[j] = w;
    }
  }
  const hmac512_key K = hmac512_key_from(kb);
  sha512_state in = K.inner;
  sha512_absorb_message<MSG_ALIGNED>(in, msg + i * stride, msg_bytes, 128);
  sha512_store(out, i, hmac512_finish(K.outer, in));
}
}  // namespace

namespace launch {
static bool word_aligned(const uint8_t* p, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(p) | stride_bytes) & 3u) == 0; }
void sha512(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n) {
  uint4* o = reinterpret_cast<uint4*>(out64);
  if (word_aligned(msg, stride_bytes)) hipLaunchKernelGGL(k_sha512<true>, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, o, n);
  else hipLaunchKernelGGL(k_sha512<false>, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, o, n);
}
void hmac_sha512(hipStream_t s, const uint8_t* key, size_t key_bytes, size_t key_stride_bytes, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n) {
  uint4* o = reinterpret_cast<uint4*>(out64);
  const bool ma = word_aligned(msg, stride_bytes), ka = word_aligned(key, key_stride_bytes);
#define HMAC512(M, K) hipLaunchKernelGGL((k_hmac_sha512<M, K>), grid_for(n), dim3(BLOCK), 0, s, key, key_bytes, key_stride_bytes, msg, msg_bytes, stride_bytes, o, n)
  if (ma && ka) HMAC512(true, true); else if (ma) HMAC512(true, false); else if (ka) HMAC512(false, true); else HMAC512(false, false);
#undef HMAC512
}
}  // namespace launch
}  // namespace ecsimd_hip
