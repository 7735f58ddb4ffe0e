// The exclusive scan of the entropy coders' per-interval byte counts -> offsets (and the total into the length word):
// three kernels defined in hhsr_jpeg.hip, launched from hhsr_png.hip as well.  sizes[n_int] uint32, totals[n_groups] uint64
// (n_groups = ceil(n_int / SCAN_GROUP)), offsets[n_int] uint64; grids: n_groups, 1, n_groups workgroups of 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ void k_jpeg_group_totals(const uint32_t* __restrict__ sizes, size_t n_int, uint64_t* __restrict__ totals);
__global__ void k_jpeg_scan_groups(uint64_t* __restrict__ totals, size_t n_groups, uint64_t* __restrict__ length);
__global__ void k_jpeg_offsets(const uint32_t* __restrict__ sizes, size_t n_int, const uint64_t* __restrict__ totals,
                               uint64_t* __restrict__ offsets);
