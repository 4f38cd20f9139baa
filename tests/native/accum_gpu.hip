// accum_gpu.hip — device harness over ptsharp_amd/csrc/pt_accum.h as it stands (tests/test_gpu_accum.py).
//
// A small shared library (tests/native/libpt_accum_check.so, built by ptsharp_amd/csrc/Makefile with the
// product's own flags) of plain C entry points.  Each copies its inputs to device 0, launches one small
// kernel over the header's functions, copies the outputs back and returns a HIP error code (or
// hipErrorInvalidValue when a size or an index is out of range: checked on the host, before any launch).
//
//   acc_to_fix        fix_ok and to_fix of n doubles
//   acc_fix_value     fix_value of n (hi, lo) pairs
//   acc_fixreg        one thread per case: up to 64 (r,g,b) terms through fixreg_add3
//   acc_add_lane      m terms, one thread each, through fix_add_lane
//   acc_add_wave      the same terms with a `has` flag through fix_add_wave without a table: 256-thread blocks,
//                     a block-uniform strided loop (as k_wf_shade_miss calls it)
//   acc_add_wave_lds  fix_add_wave with a block's LDS table, in a kernel shaped like k_wf_nee_accum
//
// The three acc_add_* read the FixAcc's raw planes w, hi and big, then run fix_take over every accumulator
// and read the planes again.  A slot with has = false (and every slot past m) carries NaN colours and the
// index of the guard accumulator, n - 1; no index is ever out of range.
//
// Restated here, not included: the dozen lines of k_wf_nee_accum (pt_wavefront.hip) that clear the LDS
// table and flush its used entries through fix_atomic after each window.  What is under test in
// acc_add_wave_lds is the header's lds_fix_add and the table path of fix_add_wave; the real flush is
// covered by the renders of tests/test_gpu_accum.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../ptsharp_amd/csrc/pt_accum.h"

using namespace pt;

namespace {

constexpr int64_t kMaxTerms = 1 << 20;   // every entry point's size cap (the tests use a few thousand)
constexpr uint32_t kWin = 16;            // k_wf_nee_accum: kAccWin rows of 256 slots per window
constexpr uint32_t kTable = 512;         // k_wf_nee_accum: kAccTable

__global__ void k_to_fix(const double* x, int64_t n, long long* v, int32_t* ok) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool o = fix_ok(x[i]);
    ok[i] = o ? 1 : 0;
    v[i] = o ? to_fix(x[i]) : 0ll;   // to_fix is defined under fix_ok only
}

__global__ void k_fix_value(const long long* hi, const unsigned long long* lo, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fix_value(hi[i], lo[i]);
}

__global__ void k_fixreg(const double* terms, const int32_t* counts, int64_t cases, unsigned long long* lo,
                         long long* hi, double* big, double* val) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cases) return;
    FixReg a;
    fixreg_clear(a);
    const double* t = terms + c * 64 * 3;
    for (int j = 0; j < counts[c]; j++) fixreg_add3(a, t[3 * j], t[3 * j + 1], t[3 * j + 2]);
    for (int k = 0; k < 3; k++) {
        lo[3 * c + k] = a.lo[k];
        hi[3 * c + k] = a.hi[k];
        big[3 * c + k] = a.big[k];
        val[3 * c + k] = fixreg_value(a, k);
    }
}

struct Terms {
    const uint32_t* idx;
    const double* rgb;          // [m][3]
    const uint8_t* has;         // [m], null: every term adds
    uint32_t m, guard;
};
struct Slot { uint32_t idx; bool has; double r, g, b; };
__device__ __forceinline__ Slot fetch(const Terms& t, uint32_t j) {
    if (j < t.m && (!t.has || t.has[j])) return Slot{t.idx[j], true, t.rgb[3 * (size_t)j], t.rgb[3 * (size_t)j + 1], t.rgb[3 * (size_t)j + 2]};
    const double q = __longlong_as_double(0x7FF8000000000000ll);
    return Slot{t.guard, false, q, q, q};
}

__global__ void k_add_lane(FixAcc A, Terms t) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < t.m) fix_add_lane(A, t.idx[j], t.rgb[3 * (size_t)j], t.rgb[3 * (size_t)j + 1], t.rgb[3 * (size_t)j + 2]);
}

__global__ __launch_bounds__(256) void k_add_wave(FixAcc A, Terms t, uint32_t* runs) {
    for (uint32_t k0 = blockIdx.x * 256u; k0 < t.m; k0 += gridDim.x * 256u) {   // block-uniform
        const uint32_t j = k0 + threadIdx.x;
        const Slot x = fetch(t, j);
        const uint32_t r = fix_add_wave(A, x.idx, x.has, x.r, x.g, x.b);
        if ((threadIdx.x & 63) == 0) runs[j >> 6] = r;
    }
}

__global__ __launch_bounds__(256) void k_add_wave_lds(FixAcc A, Terms t, uint32_t* runs) {
    __shared__ uint32_t s_key[kTable];
    __shared__ unsigned long long s_sum[kTable * 3];
    const LdsFix T{s_key, s_sum, kTable - 1u};
    for (uint32_t e = threadIdx.x; e < kTable; e += 256u) {   // restated: the clear
        s_key[e] = kLdsFree;
        s_sum[3 * e] = 0ull; s_sum[3 * e + 1] = 0ull; s_sum[3 * e + 2] = 0ull;
    }
    __syncthreads();
    for (uint32_t w0 = blockIdx.x * 256u * kWin; w0 < t.m; w0 += gridDim.x * 256u * kWin) {   // block-uniform
        for (uint32_t r = 0; r < kWin; r++) {
            const uint32_t j = w0 + r * 256u + threadIdx.x;
            const Slot x = fetch(t, j);
            const uint32_t n = fix_add_wave(A, x.idx, x.has, x.r, x.g, x.b, &T);
            if ((threadIdx.x & 63) == 0) runs[j >> 6] = n;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < kTable; e += 256u) {   // restated: the flush
            const uint32_t k = s_key[e];
            if (k == kLdsFree) continue;
            for (int c = 0; c < 3; c++) {
                const long long v = (long long)s_sum[3 * e + c];
                if (v) fix_atomic(A, k, c, v);
                s_sum[3 * e + c] = 0ull;
            }
            s_key[e] = kLdsFree;
        }
        __syncthreads();
    }
}

__global__ void k_take(FixAcc A, double* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < A.n) fix_take(A, i, out + 3 * i);
}

// Device allocations of one call, freed on every return path.
struct Pool {
    void* p[16];
    int n = 0;
    hipError_t err = hipSuccess;
    template <class T> T* get(size_t count, const T* src = nullptr) {
        void* d = nullptr;
        if (err != hipSuccess || n == 16) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
        const size_t bytes = (count ? count : 1) * sizeof(T);
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        p[n++] = d;
        err = src && count ? hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, 0, bytes);
        return (T*)d;
    }
    template <class T> void back(T* dst, const T* src, size_t count) {
        if (err == hipSuccess && count) err = hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void ran() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~Pool() { for (int i = 0; i < n; i++) (void)hipFree(p[i]); }
};

inline unsigned blocks_of(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

enum Mode { kLane = 0, kWave = 1, kWaveLds = 2 };

// planes: w [3n], hi [3n], big [3n] before fix_take and (w2, hi2, big2) after it; taken [n][3]; runs: one per
// 64-slot row of the padded slot range (kWave: 256·ceil(m/256) slots, kWaveLds: 4096·ceil(m/4096)).
int add_terms(Mode mode, const uint32_t* idx, const double* rgb, const uint8_t* has, int64_t m, int64_t n, int grid,
              unsigned long long* w, unsigned long long* hi, double* big, double* taken, unsigned long long* w2,
              unsigned long long* hi2, double* big2, uint32_t* runs) {
    if (m < 0 || m > kMaxTerms || n < 1 || n > kMaxTerms || grid < 1 || grid > 1024) return (int)hipErrorInvalidValue;
    for (int64_t j = 0; j < m; j++)
        if (idx[j] >= (uint64_t)n) return (int)hipErrorInvalidValue;
    const int64_t span = mode == kWave ? 256 : 256 * (int64_t)kWin;
    const int64_t rows = mode == kLane ? 0 : (m + span - 1) / span * (span / 64);
    hipError_t e = hipSetDevice(0);
    if (e != hipSuccess) return (int)e;
    Pool P;
    const size_t n3 = 3 * (size_t)n;
    FixAcc A{P.get<unsigned long long>(n3), P.get<unsigned long long>(n3), P.get<double>(n3), (uint64_t)n};
    Terms t{P.get(m, idx), P.get(3 * (size_t)m, rgb), has ? P.get(m, has) : nullptr, (uint32_t)m, (uint32_t)(n - 1)};
    uint32_t* d_runs = P.get<uint32_t>(rows);
    double* d_taken = P.get<double>(n3);
    if (P.err != hipSuccess) return (int)P.err;
    if (m > 0) {
        if (mode == kLane) hipLaunchKernelGGL(k_add_lane, dim3(blocks_of(m, 256)), dim3(256), 0, 0, A, t);
        else if (mode == kWave) hipLaunchKernelGGL(k_add_wave, dim3(grid), dim3(256), 0, 0, A, t, d_runs);
        else hipLaunchKernelGGL(k_add_wave_lds, dim3(grid), dim3(256), 0, 0, A, t, d_runs);
        P.ran();
    }
    P.back(w, A.w, n3); P.back(hi, A.hi, n3); P.back(big, A.big, n3);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_take, dim3(blocks_of(n, 256)), dim3(256), 0, 0, A, d_taken);
    P.ran();
    P.back(taken, d_taken, n3);
    P.back(w2, A.w, n3); P.back(hi2, A.hi, n3); P.back(big2, A.big, n3);
    if (runs) P.back(runs, d_runs, (size_t)rows);
    return (int)P.err;
}

}  // namespace

extern "C" {

int acc_to_fix(const double* x, int64_t n, long long* v, int32_t* ok) {
    if (n < 1 || n > kMaxTerms) return (int)hipErrorInvalidValue;
    hipError_t e = hipSetDevice(0);
    if (e != hipSuccess) return (int)e;
    Pool P;
    const double* dx = P.get(n, x);
    long long* dv = P.get<long long>(n);
    int32_t* dok = P.get<int32_t>(n);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_to_fix, dim3(blocks_of(n, 256)), dim3(256), 0, 0, dx, n, dv, dok);
    P.ran();
    P.back(v, dv, n); P.back(ok, dok, n);
    return (int)P.err;
}

int acc_fix_value(const long long* hi, const unsigned long long* lo, int64_t n, double* out) {
    if (n < 1 || n > kMaxTerms) return (int)hipErrorInvalidValue;
    hipError_t e = hipSetDevice(0);
    if (e != hipSuccess) return (int)e;
    Pool P;
    const long long* dhi = P.get(n, hi);
    const unsigned long long* dlo = P.get(n, lo);
    double* dout = P.get<double>(n);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_fix_value, dim3(blocks_of(n, 256)), dim3(256), 0, 0, dhi, dlo, n, dout);
    P.ran();
    P.back(out, dout, n);
    return (int)P.err;
}

// terms [cases][64][3], counts [cases] (each 0..64); lo, hi, big, val [cases][3]
int acc_fixreg(const double* terms, const int32_t* counts, int64_t cases, unsigned long long* lo, long long* hi,
               double* big, double* val) {
    if (cases < 1 || cases > 4096) return (int)hipErrorInvalidValue;
    for (int64_t c = 0; c < cases; c++)
        if (counts[c] < 0 || counts[c] > 64) return (int)hipErrorInvalidValue;
    hipError_t e = hipSetDevice(0);
    if (e != hipSuccess) return (int)e;
    Pool P;
    const size_t c3 = 3 * (size_t)cases;
    const double* dt = P.get((size_t)cases * 64 * 3, terms);
    const int32_t* dc = P.get(cases, counts);
    unsigned long long* dlo = P.get<unsigned long long>(c3);
    long long* dhi = P.get<long long>(c3);
    double* dbig = P.get<double>(c3);
    double* dval = P.get<double>(c3);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_fixreg, dim3(blocks_of(cases, 64)), dim3(64), 0, 0, dt, dc, cases, dlo, dhi, dbig, dval);
    P.ran();
    P.back(lo, dlo, c3); P.back(hi, dhi, c3); P.back(big, dbig, c3); P.back(val, dval, c3);
    return (int)P.err;
}

int acc_add_lane(const uint32_t* idx, const double* rgb, int64_t m, int64_t n, unsigned long long* w,
                 unsigned long long* hi, double* big, double* taken, unsigned long long* w2, unsigned long long* hi2,
                 double* big2) {
    return add_terms(kLane, idx, rgb, nullptr, m, n, 1, w, hi, big, taken, w2, hi2, big2, nullptr);
}

int acc_add_wave(const uint32_t* idx, const double* rgb, const uint8_t* has, int64_t m, int64_t n, int grid,
                 unsigned long long* w, unsigned long long* hi, double* big, double* taken, unsigned long long* w2,
                 unsigned long long* hi2, double* big2, uint32_t* runs) {
    if (!has || !runs) return (int)hipErrorInvalidValue;
    return add_terms(kWave, idx, rgb, has, m, n, grid, w, hi, big, taken, w2, hi2, big2, runs);
}

int acc_add_wave_lds(const uint32_t* idx, const double* rgb, const uint8_t* has, int64_t m, int64_t n, int grid,
                     unsigned long long* w, unsigned long long* hi, double* big, double* taken,
                     unsigned long long* w2, unsigned long long* hi2, double* big2, uint32_t* runs) {
    if (!has || !runs) return (int)hipErrorInvalidValue;
    return add_terms(kWaveLds, idx, rgb, has, m, n, grid, w, hi, big, taken, w2, hi2, big2, runs);
}

}  // extern "C"
