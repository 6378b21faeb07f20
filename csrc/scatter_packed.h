// Kernel-argument region table of scatter_append_packed (K16, packed form),
// shared by the kernel (kernels.hip) and its torch binding (hip_ops.cpp).

#pragma once

#include <cstdint>

namespace gdb_hip {

constexpr int kPackedRegions = 16;

// Destinations of up to kPackedRegions region memtables, passed by value:
// 5 * 16 * 8 = 640 bytes of kernel arguments, no device-side pointer table.
struct PackedRegions {
  int64_t* ts[kPackedRegions];
  int32_t* se[kPackedRegions];
  double* f[kPackedRegions];        // fields [nf, stride] row-major
  int64_t stride[kPackedRegions];   // field row stride (memtable capacity)
  int64_t base[kPackedRegions];     // first free row before this batch
};

}  // namespace gdb_hip
