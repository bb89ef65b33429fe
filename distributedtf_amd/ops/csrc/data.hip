// On-device input pipelines.  CIFAR: gather + pad/crop/flip augmentation + per-image standardization + cast/pack,
// in one launch (reference: cifar10_main.py:71-109 preprocess_image / parse_record, which TF runs on the CPU
// through tf.data; here the uint8 dataset lives in HBM and a batch is produced without leaving the GPU).
//
//   one wave per image: 1024 pixels = 16 per lane, the 48 channel values stay in VGPRs for the two-pass
//   mean / variance (tf.image.per_image_standardization: (x - mean) / max(std, 1/sqrt(N)), N = 3072).
//   Random crop offsets and the flip bit come from a counter-based hash of (seed, counter, batch position);
//   seed/counter are read from device memory so a captured HIP graph draws new crops on every replay.  With
//   per-member keys (key_slot != null: the population step's images) the hash is of (seed, the member's own step
//   counter read from its state row, dataset row) instead: a member's crops then depend only on the member -- not on
//   which other members share its plan, its position in the packed batch, or how many launches its rank ran -- so a
//   PBT run draws the same augmentation at any placement of the population over ranks (tests/test_gpu_placement.py).
//   Outputs: bf16 NHWC with channels zero-padded to 16 (the HIP ResNet stem input) and/or fp32 NHWC (C=3).
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

constexpr int IMG = 32, PAD = 4, CH = 3, NPIX = IMG * IMG, PPL = NPIX / 64;

__global__ __launch_bounds__(256) void augment_cifar_kernel(const uint8_t* __restrict__ images,
                                                            const long* __restrict__ labels_src,
                                                            const long* __restrict__ idx,
                                                            const uint32_t* __restrict__ rng, int n, int augment,
                                                            bf16_t* __restrict__ out16, float* __restrict__ out32,
                                                            int* __restrict__ lab32, long* __restrict__ lab64,
                                                            const int* __restrict__ key_slot,
                                                            const float* __restrict__ key_state, long key_stride,
                                                            long key_col) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const long src = idx[p];
  int oy = PAD, ox = PAD, flip = 0;
  if (augment) {
    const uint32_t h =
        key_slot != nullptr
            ? mix32(rng[0] ^ mix32((uint32_t)(int)key_state[(long)key_slot[p] * key_stride + key_col] * 0x9E3779B9u +
                                   (uint32_t)src))
            : mix32(rng[0] ^ mix32(rng[1] * 0x9E3779B9u + (uint32_t)p));
    oy = (int)(h % 9u);
    ox = (int)((h >> 8) % 9u);
    flip = (int)((h >> 16) & 1u);
  }
  const uint8_t* im = images + src * (long)(NPIX * CH);
  float v[PPL][CH];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int q = lane + 64 * j;
    const int y = q >> 5, x = q & 31;
    const int sy = y + oy - PAD;
    const int sx = (flip ? IMG - 1 - x : x) + ox - PAD;
    const bool in = (unsigned)sy < (unsigned)IMG && (unsigned)sx < (unsigned)IMG;
    const uint8_t* px = im + (sy * IMG + sx) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      v[j][c] = in ? (float)px[c] : 0.f;
      s += v[j][c];
    }
  }
  const float mean = wave_sum(s) * (1.f / (NPIX * CH));
  float q2 = 0.f;
#pragma unroll
  for (int j = 0; j < PPL; ++j)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const float d = v[j][c] - mean;
      q2 += d * d;
    }
  const float var = wave_sum(q2) * (1.f / (NPIX * CH));
  const float adj = fmaxf(sqrtf(var), rsqrtf((float)(NPIX * CH)));
  const float inv = 1.f / adj;
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int q = lane + 64 * j;
    const float a = (v[j][0] - mean) * inv, b = (v[j][1] - mean) * inv, c = (v[j][2] - mean) * inv;
    if (out16) {
      uint4* dst = reinterpret_cast<uint4*>(out16 + ((long)p * NPIX + q) * 16);
      dst[0] = make_uint4(pack2bf(a, b), pack2bf(c, 0.f), 0u, 0u);
      dst[1] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (out32) {
      float* d = out32 + ((long)p * NPIX + q) * CH;
      d[0] = a;
      d[1] = b;
      d[2] = c;
    }
  }
  if (lane == 0) {
    const long l = labels_src[src];
    if (lab32) lab32[p] = (int)l;
    if (lab64) lab64[p] = l;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// ImageNet-style input path: gather + random-resized crop (or the evaluation central crop) + bilinear resample to
// H x H + horizontal flip + channel-mean subtraction + cast/pack, in one launch.  The dataset is uint8 NHWC with a
// square stored side S.
//
//   The crop box is drawn with integer arithmetic only (datasets.imagenet_augment_params mirrors it bit for bit):
//   up to 10 attempts, each from a re-hashed word h -- area = S^2 * f with f in [0.08, 1) as Q16 from h's low 16
//   bits, aspect ratio w / h from a 16-entry Q16 table of log-spaced ratios 3/4 .. 4/3 (entry 15 - i is the
//   reciprocal of entry i) indexed by bits 16..19, w = isqrt(area * r), h = isqrt(area / r); the first attempt with
//   1 <= w, h <= S is placed by a second hash, else the box is the whole image.  The flip bit is bit 20 of the first
//   word.  The keys are those of augment_cifar_kernel.  augment = 0: the central crop of side round(0.875 S), no
//   flip (resize-256 / crop-224 evaluation on square stored images).
//
//   Resample: src = (o + 0.5) * crop / H - 0.5 + origin clamped to the box (half-pixel centres, the convention of
//   interpolate(mode="bilinear", align_corners=False)); the position relative to the box origin is the integer
//   (2 o + 1) * crop - H over 2 H, clamped, then a correctly rounded fp32 division (one per row and per column of
//   the block, four per thread): exact for an integer or half-integer position, and its floor is the exact floor
//   for (2 H + 1) S < 2^23.  A multiply by a precomputed 1 / (2 H) is cheaper but not exact there, so the
//   division stays.
//   value = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11) - mean[c] in fp32, rounded once.
//
//   One wave per 64 2x2 output blocks of one image, so the box, the scale and the means are wave-uniform: the wave
//   index goes through readfirstlane on purpose, so that idx[p], the label, the rng words, the member key and the
//   ratio table are read once per wave through the scalar cache and the whole box rule runs on the scalar unit
//   (read-only data of this launch; nothing is written through the scalar path).  The pixels are per-lane byte
//   loads at unaligned addresses, 48 per thread (4 taps x 4 pixels x 3 channels; the compiler pairs neighbours
//   into ushort + ubyte loads): RGB triples at a computed position have no wider alignment.  A thread
//   writes its block as two 16-byte stores of the space-to-depth layout [n, H/2, H/2, 16] (channel (2 dy + dx) * 3 + c,
//   12..15 zero), one 16-byte store per pixel of the padded layout [n, H, H, 8] (3..7 zero), and / or fp32 [n, H, H, 3].
constexpr uint32_t IMN_RATIO_Q16[16] = {49152u, 51074u, 53071u, 55146u, 57303u, 59543u, 61872u, 64291u,
                                        66805u, 69417u, 72132u, 74952u, 77883u, 80929u, 84093u, 87381u};
constexpr uint32_t IMN_AREA_MIN_Q16 = 5243u;  // ceil(0.08 * 65536)
constexpr int IMN_ATTEMPTS = 10;

__device__ __forceinline__ uint32_t isqrt32(uint32_t v) {  // floor(sqrt(v)), v < 2^30
  uint32_t r = 0;
#pragma unroll
  for (int b = 14; b >= 0; --b) {
    const uint32_t t = r | (1u << b);
    if (t * t <= v) r = t;
  }
  return r;
}

// One body, two entry points.  STAGED = false (dtf_augment_imagenet): image p of the launch is images[idx[p]], the
// set lives on the device.  STAGED = true (dtf_augment_imagenet_staged): the set's pixels live on the host and image p
// was copied to stage[half][p] of a two-half staging tensor [2][cap][S][S][3] before the launch; half (0 or 1) is read
// from a one-word device tensor -- one more wave-uniform scalar load, no more loads per pixel --, so one captured
// graph serves both halves.  idx[p] is still the dataset row: it keys the draw and selects the label, never a pixel.
template <bool STAGED>
__global__ __launch_bounds__(256) void augment_imagenet_kernel(
    const uint8_t* __restrict__ images, const int* __restrict__ half_word, long cap,
    const long* __restrict__ labels_src, const long* __restrict__ idx,
    const uint32_t* __restrict__ rng, int n, long nrows, int S, int H, int augment, bf16_t* __restrict__ out_s2d,
    bf16_t* __restrict__ out_pad, float* __restrict__ out32, int* __restrict__ lab32, long* __restrict__ lab64,
    int* __restrict__ boxes, const int* __restrict__ key_slot, const float* __restrict__ key_state, long key_stride,
    long key_col) {
  const int lane = threadIdx.x & 63;
  const int Hb = H >> 1;
  const int nblk = Hb * Hb;
  const int cpi = (nblk + 63) >> 6;  // 64-block chunks per image
  const int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int p = wv / cpi;
  if (p >= n) return;
  const int chunk = wv - p * cpi;
  long src = idx[p];
  src = src < 0 ? 0 : (src >= nrows ? nrows - 1 : src);  // a bad index reads a valid row, never out of bounds
  // ---- the box (wave-uniform)
  int y0, x0, bh, bw, flip = 0;
  if (augment) {
    uint32_t h =
        key_slot != nullptr
            ? mix32(rng[0] ^ mix32((uint32_t)(int)key_state[(long)key_slot[p] * key_stride + key_col] * 0x9E3779B9u +
                                   (uint32_t)src))
            : mix32(rng[0] ^ mix32(rng[1] * 0x9E3779B9u + (uint32_t)p));
    flip = (int)((h >> 20) & 1u);
    y0 = x0 = 0;
    bh = bw = S;  // no attempt fits: the whole image
    const uint64_t A = (uint64_t)S * (uint64_t)S;
    for (int t = 0; t < IMN_ATTEMPTS; ++t) {
      const uint32_t f = IMN_AREA_MIN_Q16 + (((h & 0xffffu) * (65536u - IMN_AREA_MIN_Q16)) >> 16);
      const uint64_t area = (A * f) >> 16;
      const int r = (int)((h >> 16) & 15u);
      const uint32_t w = isqrt32((uint32_t)((area * IMN_RATIO_Q16[r]) >> 16));
      const uint32_t hh = isqrt32((uint32_t)((area * IMN_RATIO_Q16[15 - r]) >> 16));
      if (w >= 1u && hh >= 1u && w <= (uint32_t)S && hh <= (uint32_t)S) {
        const uint32_t g = mix32(h ^ 0x68E31DA4u);
        bh = (int)hh;
        bw = (int)w;
        y0 = (int)(((g & 0xffffu) * (uint32_t)(S - bh + 1)) >> 16);
        x0 = (int)(((g >> 16) * (uint32_t)(S - bw + 1)) >> 16);
        break;
      }
      h = mix32(h + 0x9E3779B9u);
    }
  } else {
    bh = bw = (7 * S + 4) >> 3;  // round(0.875 S)
    y0 = x0 = (S - bh) >> 1;
  }
  if (chunk == 0 && lane == 0) {
    const long l = labels_src[src];
    if (lab32) lab32[p] = (int)l;
    if (lab64) lab64[p] = l;
    if (boxes) {
      int* b = boxes + (long)p * 5;
      b[0] = y0, b[1] = x0, b[2] = bh, b[3] = bw, b[4] = flip;
    }
  }
  const int blk = chunk * 64 + lane;
  if (blk >= nblk) return;
  const int by = blk / Hb, bx = blk - by * Hb;
  // ---- sample positions of the block's two rows and two columns: taps i, i + 1 (clamped) and the weight of i + 1
  const float den = (float)(2 * H);
  int ty[2][2], tx[2][2];
  float fy[2], fx[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int oy = 2 * by + d;
    const int oxo = 2 * bx + d;
    const int ox = flip ? H - 1 - oxo : oxo;
    int ny = (2 * oy + 1) * bh - H, nx = (2 * ox + 1) * bw - H;
    ny = min(max(ny, 0), (bh - 1) * 2 * H);
    nx = min(max(nx, 0), (bw - 1) * 2 * H);
    const float qy = (float)ny / den, qx = (float)nx / den;
    const int iy = (int)qy, ix = (int)qx;
    fy[d] = qy - (float)iy;
    fx[d] = qx - (float)ix;
    ty[d][0] = y0 + iy;
    ty[d][1] = y0 + min(iy + 1, bh - 1);
    tx[d][0] = x0 + ix;
    tx[d][1] = x0 + min(ix + 1, bw - 1);
  }
  // staged: the launch's image p of the half named by the device word (masked: a bad word cannot leave the tensor)
  const long img = STAGED ? (long)(half_word[0] & 1) * cap + p : src;
  const uint8_t* im = images + img * ((long)S * S * CH);
  const float mean[CH] = {123.68f, 116.78f, 103.94f};
  float v[2][2][CH];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const uint8_t* p00 = im + ((long)ty[dy][0] * S + tx[dx][0]) * CH;
      const uint8_t* p01 = im + ((long)ty[dy][0] * S + tx[dx][1]) * CH;
      const uint8_t* p10 = im + ((long)ty[dy][1] * S + tx[dx][0]) * CH;
      const uint8_t* p11 = im + ((long)ty[dy][1] * S + tx[dx][1]) * CH;
      const float wx = fx[dx], wy = fy[dy];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const float top = (1.f - wx) * (float)p00[c] + wx * (float)p01[c];
        const float bot = (1.f - wx) * (float)p10[c] + wx * (float)p11[c];
        v[dy][dx][c] = ((1.f - wy) * top + wy * bot) - mean[c];
      }
    }
  if (out_s2d) {
    uint4* dst = reinterpret_cast<uint4*>(out_s2d + ((long)p * nblk + blk) * 16);
    dst[0] = make_uint4(pack2bf(v[0][0][0], v[0][0][1]), pack2bf(v[0][0][2], v[0][1][0]),
                        pack2bf(v[0][1][1], v[0][1][2]), pack2bf(v[1][0][0], v[1][0][1]));
    dst[1] = make_uint4(pack2bf(v[1][0][2], v[1][1][0]), pack2bf(v[1][1][1], v[1][1][2]), 0u, 0u);
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const long pix = ((long)p * H + (2 * by + dy)) * H + 2 * bx;
    if (out_pad) {
      uint4* dst = reinterpret_cast<uint4*>(out_pad + pix * 8);
      dst[0] = make_uint4(pack2bf(v[dy][0][0], v[dy][0][1]), pack2bf(v[dy][0][2], 0.f), 0u, 0u);
      dst[1] = make_uint4(pack2bf(v[dy][1][0], v[dy][1][1]), pack2bf(v[dy][1][2], 0.f), 0u, 0u);
    }
    if (out32) {
      float2* dst = reinterpret_cast<float2*>(out32 + pix * CH);  // 6 floats at an even pixel: 8-byte aligned
      dst[0] = make_float2(v[dy][0][0], v[dy][0][1]);
      dst[1] = make_float2(v[dy][0][2], v[dy][1][0]);
      dst[2] = make_float2(v[dy][1][1], v[dy][1][2]);
    }
  }
}

}  // namespace

// Host-side argument check of dtf_augment_imagenet: the sizes at which the kernel's integer positions stay exact in
// fp32 ((2 o + 1) * crop < 2^23) and its int offsets cannot overflow.
// cap >= 0: the staged form's images per staging half, which must hold the launch (n <= cap).
static bool imagenet_args_ok(int n, long nrows, int S, int H, long cap = -1) {
  if (n < 0 || nrows < 1 || S < 1 || S > 4096 || H < 2 || (H & 1) || H > 1024) return false;
  if (cap >= 0 && (n > cap || cap < 1)) return false;
  if ((long)(2 * H + 1) * S >= (1L << 23)) return false;
  const long cpi = ((long)(H / 2) * (H / 2) + 63) / 64;
  return (long)n * cpi < (1L << 31) - 4;
}

DTF_API int dtf_augment_imagenet(const uint8_t* images, const long* labels_src, const long* idx, const uint32_t* rng,
                                 int n, long nrows, int S, int H, int augment, bf16_t* out_s2d, bf16_t* out_pad,
                                 float* out32, int* lab32, long* lab64, int* boxes, const int* key_slot,
                                 const float* key_state, long key_stride, long key_col, hipStream_t stream) {
  if (!imagenet_args_ok(n, nrows, S, H)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long cpi = ((long)(H / 2) * (H / 2) + 63) / 64;
  hipLaunchKernelGGL(augment_imagenet_kernel<false>, dim3((unsigned)((n * cpi + 3) / 4)), dim3(256), 0, stream, images,
                     (const int*)nullptr, 0L, labels_src, idx, rng, n, nrows, S, H, augment, out_s2d, out_pad, out32,
                     lab32, lab64, boxes, key_slot, key_state, key_stride, key_col);
  return DTF_CHECK_LAUNCH();
}

// The staged form (augment_imagenet_kernel<true>): stage [2][cap][S][S][3] uint8, half_word one int32 on the device
// (0 or 1); nrows is the dataset's row count (labels_src, the clamp of idx).  n images need n <= cap.
DTF_API int dtf_augment_imagenet_staged(const uint8_t* stage, const int* half_word, long cap, const long* labels_src,
                                        const long* idx, const uint32_t* rng, int n, long nrows, int S, int H,
                                        int augment, bf16_t* out_s2d, bf16_t* out_pad, float* out32, int* lab32,
                                        long* lab64, int* boxes, const int* key_slot, const float* key_state,
                                        long key_stride, long key_col, hipStream_t stream) {
  if (!imagenet_args_ok(n, nrows, S, H, cap)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const long cpi = ((long)(H / 2) * (H / 2) + 63) / 64;
  hipLaunchKernelGGL(augment_imagenet_kernel<true>, dim3((unsigned)((n * cpi + 3) / 4)), dim3(256), 0, stream, stage,
                     half_word, cap, labels_src, idx, rng, n, nrows, S, H, augment, out_s2d, out_pad, out32, lab32,
                     lab64, boxes, key_slot, key_state, key_stride, key_col);
  return DTF_CHECK_LAUNCH();
}

DTF_API int dtf_augment_cifar(const uint8_t* images, const long* labels_src, const long* idx, const uint32_t* rng,
                              int n, int augment, bf16_t* out16, float* out32, int* lab32, long* lab64,
                              const int* key_slot, const float* key_state, long key_stride, long key_col,
                              hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(augment_cifar_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, images, labels_src, idx, rng, n,
                     augment, out16, out32, lab32, lab64, key_slot, key_state, key_stride, key_col);
  return DTF_CHECK_LAUNCH();
}
