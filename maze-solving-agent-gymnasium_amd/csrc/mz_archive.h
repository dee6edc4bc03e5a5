// mz_archive.h — what mz_archive.hip shares with the rest of the library: the handle as entry
// points outside mz_api.hip see it (mz_api.hip owns struct mz_handle), the C ABI's error string
// and device guard, and the launch geometry of an importing build (mz_env.hip).
#pragma once
#include "../../include/mazerl.h"
#include "mz_common.h"

const MzDev& mz_handle_dev(const mz_handle* h);
int mz_handle_device(const mz_handle* h);
int mz_fail_msg(int code, const char* msg);  // sets mz_last_error(), returns code

// k_build's launch geometry for an import (mz_env.hip): dynamic LDS bytes, the attribute a
// kernel needs above 64 KiB of it, and the persistent grid for n mazes
size_t mz_import_lds(int P, bool tor);
hipError_t mz_build_lds_attr(const void* fn, size_t bytes);
int mz_build_launch_grid(int n, size_t lds);

struct MzDeviceGuard {  // run a call on the handle's device, restore the caller's afterwards
  int prev = -1;
  explicit MzDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~MzDeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// int32 words of one archive entry's bit field for pitch P: ceil(P * P / 32)
__host__ __device__ inline int mz_archive_entry_words(int P) { return (P * P + 31) / 32; }
