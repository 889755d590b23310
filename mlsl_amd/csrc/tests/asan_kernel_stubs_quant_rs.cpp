// Host-only stubs for the quantized reduce-scatter's epilogue launchers; see
// asan_kernel_stubs.cpp. Any call is a hard error.
#include "../core/types.hpp"
#include "../hip/kernels.hpp"

namespace mlsl {
#define STUB(...) { MLSL_THROW("kernel launcher called in host-only ASan build"); }
void LaunchQuantSumDequant(const void*, const void*, void*, size_t, size_t, DataType, hipStream_t) STUB()
void LaunchQuantSumDequantNT(const void*, const void*, void*, size_t, size_t, DataType, hipStream_t) STUB()
}  // namespace mlsl
