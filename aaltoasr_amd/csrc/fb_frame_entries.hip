// fb_frame_entries.hip -- the forward-backward pass's per-frame pdf occupancies as weighted entries grouped by frame, on
// the device.  Layout and order: fb_frame_entries.h.  Every value has one lane and one fixed order of operations; the
// only sums across lanes are the integer prefix sums of the offsets.
#include <hip/hip_runtime.h>

#include "common.h"
#include "fb_frame_entries.h"

namespace aasr {

__global__ __launch_bounds__(FBF_THREADS) void k_fb_frame_counts(const FbEntryUtt *__restrict__ utt,
                                                                 const double *__restrict__ occ,
                                                                 int32_t *__restrict__ counts) {
  const FbEntryUtt u = utt[blockIdx.y];
  const int t = blockIdx.x * FBF_THREADS + threadIdx.x;
  if (t >= u.T) return;
  const double *o = occ + u.occ + (int64_t)t * u.n_pdf;
  int32_t n = 0;
  for (int j = 0; j < u.n_pdf; j++) n += o[j] > 0 ? 1 : 0;
  counts[u.row0 + t] = n;
}

// inclusive prefix sums of one value per thread over the workgroup, in place in `lds`; -> the thread's inclusive sum
__device__ inline int64_t fbf_block_scan(int64_t v, int64_t *lds) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int d = 1; d < FBF_THREADS; d <<= 1) {
    const int64_t a = tid >= d ? lds[tid - d] : 0;
    __syncthreads();
    lds[tid] += a;
    __syncthreads();
  }
  return lds[tid];
}

// rows [b FBF_SCAN_ROWS ...): off[r] = the sum of the block's counts before r; block_sums[b] = the block's total
__global__ __launch_bounds__(FBF_THREADS) void k_fb_frame_scan_block(const int32_t *__restrict__ counts, int64_t n_rows,
                                                                     int64_t *__restrict__ block_sums,
                                                                     int64_t *__restrict__ off) {
  __shared__ int64_t lds[FBF_THREADS];
  const int64_t r0 = ((int64_t)blockIdx.x * FBF_THREADS + threadIdx.x) * FBF_SCAN_ITEMS;
  int64_t c[FBF_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int i = 0; i < FBF_SCAN_ITEMS; i++) {
    c[i] = r0 + i < n_rows ? counts[r0 + i] : 0;
    s += c[i];
  }
  int64_t at = fbf_block_scan(s, lds) - s;
#pragma unroll
  for (int i = 0; i < FBF_SCAN_ITEMS; i++) {
    if (r0 + i <= n_rows) off[r0 + i] = at;
    at += c[i];
  }
  if (threadIdx.x == FBF_THREADS - 1) block_sums[blockIdx.x] = lds[FBF_THREADS - 1];
}

// one workgroup: block_sums[b] = the total of the blocks before b, FBF_THREADS blocks a step with a carry
__global__ __launch_bounds__(FBF_THREADS) void k_fb_frame_scan_top(int64_t *__restrict__ block_sums, int64_t n_blocks) {
  __shared__ int64_t lds[FBF_THREADS];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_blocks; base += FBF_THREADS) {
    const int64_t b = base + threadIdx.x;
    const int64_t v = b < n_blocks ? block_sums[b] : 0;
    const int64_t inc = fbf_block_scan(v, lds);
    if (b < n_blocks) block_sums[b] = carry + inc - v;
    carry += lds[FBF_THREADS - 1];
    __syncthreads();  // (the next step rewrites lds)
  }
}

__global__ __launch_bounds__(FBF_THREADS) void k_fb_frame_scan_add(const int64_t *__restrict__ block_sums, int64_t n_rows,
                                                                   int64_t *__restrict__ off) {
  const int64_t r = (int64_t)blockIdx.x * FBF_THREADS + threadIdx.x;
  if (r > n_rows) return;
  off[r] += block_sums[r / FBF_SCAN_ROWS];
}

__global__ __launch_bounds__(FBF_THREADS) void k_fb_frame_fill(const FbEntryUtt *__restrict__ utt,
                                                               const int64_t *__restrict__ pdf_at,
                                                               const int32_t *__restrict__ pdfs,
                                                               const double *__restrict__ occ,
                                                               const double *__restrict__ sums,
                                                               const int64_t *__restrict__ off, int32_t *__restrict__ pdf,
                                                               double *__restrict__ weight) {
  const FbEntryUtt u = utt[blockIdx.y];
  const int t = blockIdx.x * FBF_THREADS + threadIdx.x;
  if (t >= u.T) return;
  const double *o = occ + u.occ + (int64_t)t * u.n_pdf;
  const int32_t *list = pdfs + pdf_at[blockIdx.y];
  const double s = sums[u.sums + t];
  int64_t at = off[u.row0 + t];
  const int64_t end = off[u.row0 + t + 1];  // the count pass found as many entries: nothing is written past them
  for (int j = 0; j < u.n_pdf && at < end; j++) {
    const double g = o[j];
    if (!(g > 0)) continue;
    pdf[at] = list[j];
    weight[at] = g / s;
    at++;
  }
}

void fb_frame_counts_launch(const FbEntryUtt *utt, int32_t n_utt, int32_t max_T, const double *occ, int32_t *counts,
                            hipStream_t stream) {
  if (n_utt <= 0 || max_T <= 0) return;
  hipLaunchKernelGGL(k_fb_frame_counts, dim3((unsigned)((max_T + FBF_THREADS - 1) / FBF_THREADS), (unsigned)n_utt),
                     dim3(FBF_THREADS), 0, stream, utt, occ, counts);
  AASR_HIP(hipGetLastError());
}

void fb_frame_offsets_launch(const int32_t *counts, int64_t n_rows, int64_t *block_sums, int64_t *off, hipStream_t stream) {
  if (n_rows < 0) return;
  const int64_t blocks = fb_frame_scan_blocks(n_rows);
  hipLaunchKernelGGL(k_fb_frame_scan_block, dim3((unsigned)blocks), dim3(FBF_THREADS), 0, stream, counts, n_rows, block_sums,
                     off);
  AASR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fb_frame_scan_top, dim3(1), dim3(FBF_THREADS), 0, stream, block_sums, blocks);
  AASR_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fb_frame_scan_add, dim3((unsigned)((n_rows + 1 + FBF_THREADS - 1) / FBF_THREADS)), dim3(FBF_THREADS), 0,
                     stream, block_sums, n_rows, off);
  AASR_HIP(hipGetLastError());
}

void fb_frame_fill_launch(const FbEntryUtt *utt, const int64_t *pdf_at, const int32_t *pdfs, int32_t n_utt, int32_t max_T,
                          const double *occ, const double *sums, const int64_t *off, int32_t *pdf, double *weight,
                          hipStream_t stream) {
  if (n_utt <= 0 || max_T <= 0) return;
  hipLaunchKernelGGL(k_fb_frame_fill, dim3((unsigned)((max_T + FBF_THREADS - 1) / FBF_THREADS), (unsigned)n_utt),
                     dim3(FBF_THREADS), 0, stream, utt, pdf_at, pdfs, occ, sums, off, pdf, weight);
  AASR_HIP(hipGetLastError());
}

}  // namespace aasr
