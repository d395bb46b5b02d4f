// exact-f32 MFMA tile kernels (fp32 parity mode)
#include "kx_gemm_impl.h"

int kx_gemm_launch_f32(GemmParams& p, const KxGemmPlan& k, const KxTuning& tn, hipStream_t s) {
  const int tile = k.tile;
  if (tile == 16) return kx_gemm_launch_gemv_f32(p, tn, s);
  if (tile == 128) return launch<float, 128, 128>(p, k, s);
  if (tile == 64) return launch<float, 64, 64>(p, k, s);
  kx_set_error("kx_gemm: unknown tile variant %d", tile);
  return KX_ERR_UNSUPPORTED;
}
