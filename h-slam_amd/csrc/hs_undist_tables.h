// hs_undist_tables.h — host-only helpers of the undistortion tables (hs_undist_tables.cpp; plain C++17, no HIP).
#pragma once
#include <cstddef>

// HS_OK when every entry of a caller's map is finite and within +-32767 (the kernel's fixed-point range: the
// coordinate times 32 must round into an int with room to spare), else HS_ERR_INVALID with hs_last_error set.
int hs_undist_check_map(const float* remap_x, const float* remap_y, size_t n);
