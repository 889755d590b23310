// Host-only stub for the one-shot quantized reduce-scatter's fan-in launcher;
// see asan_kernel_stubs.cpp. Any call is a hard error.
#include "../core/types.hpp"
#include "../hip/kernels.hpp"

namespace mlsl {
#define STUB(...) { MLSL_THROW("kernel launcher called in host-only ASan build"); }
void LaunchQuantSumDequantN(const void* const*, int, void*, size_t, size_t, DataType, hipStream_t) STUB()
}  // namespace mlsl
