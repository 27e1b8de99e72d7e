// Does the SHAPE of the row loads bound k_enc_select_runs<8, 2>?  Two kernels over the same 8192 pages of 65 536 Float64 rows,
// same geometry as the shipped kernel (one workgroup of 256 per page, __launch_bounds__(256, 4), 40 KB of LDS so that four
// workgroups share a CU, chunks of 4096 rows, 16 rows per thread): each loads a chunk, compares every row with the row
// before it and counts the changes.  Nothing else of the selector is here.
//   (a) rows as the selector has loaded them so far: thread t holds rows 16t .. 16t + 15, eight 16-byte loads at a lane stride
//       of 128 bytes — a wave-level load touches 64 lines and takes 16 bytes of each;
//   (b) lane-contiguous: piece u of lane l holds rows 1024w + 128u + 2l + {0, 1} — a wave-level load is 1 KiB contiguous,
//       8 lines; the row before a lane's piece comes from the lane below (DPP wave shift), the compares are wave-wide ballots.
// The two change totals must agree.  Ten launches each, timed one by one with HIP events.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/micro/runs_loads.hip -o scripts/micro/bin/runs_loads
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int WG = 256, K = 16;
constexpr uint32_t CHUNK = WG * K;
constexpr uint32_t PAD_WORDS = 10200;  // 40.8 KB as the shipped kernel: four workgroups per CU, not five

#define CK(x)                                                                          \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
// runs of 1 .. 63 rows: every block of 32 rows is cut once at a hashed position, each part takes one of 256 values
__global__ void k_fill(double* v, uint64_t rows) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t b = (uint32_t)(r >> 5), cut = mix(b) & 31;
    v[r] = (double)(mix(2 * b + ((uint32_t)(r & 31) >= cut) + 0x9E3779B9u) & 255);
}

__device__ __forceinline__ u32x4 ldu128(const uint8_t* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
// lane l takes lane l - 1's value, lane 0 takes `lane0` (v_mov_b32 with DPP wave_shr:1 keeps the old value where no lane feeds it)
__device__ __forceinline__ uint64_t wave_shr1(uint64_t v, uint64_t lane0) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)lane0, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(lane0 >> 32), (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

template <int LANE_ROWS>
__global__ void __launch_bounds__(WG, 4) k_loads(const uint8_t* base, uint64_t N, uint32_t* out) {
    __shared__ uint32_t pad[PAD_WORDS];
    __shared__ uint32_t s_total;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint8_t* vals = base + (uint64_t)blockIdx.x * N * 8;
    for (uint32_t i = t; i < PAD_WORDS; i += WG) pad[i] = i;
    if (t == 0) s_total = 0;
    __syncthreads();
    uint32_t changes = 0;
    for (uint64_t cb = 0; cb < N; cb += CHUNK) {  // (N is a multiple of CHUNK here)
        uint64_t v[K];
        if constexpr (!LANE_ROWS) {
            const uint32_t r0 = (uint32_t)t * K;
            u32x4 q[K / 2];
#pragma unroll
            for (int u = 0; u < K / 2; u++) q[u] = ldu128(vals + (cb + r0) * 8 + 16 * u);
            __builtin_memcpy(v, q, sizeof v);
            uint64_t pv0 = 0;
            if (lane == 0) pv0 = ld64(vals + (cb + r0 > 0 ? cb + r0 - 1 : 0) * 8);
            uint64_t pr = __shfl(v[K - 1], (lane + 63) & 63, 64);
            if (lane == 0) pr = pv0;
            uint32_t rbm = 0;
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (v[j] != pr) rbm |= 1u << j;
                pr = v[j];
            }
            changes += (uint32_t)__popc(rbm);
        } else {
            const uint32_t wrow = (uint32_t)w * 1024;
#pragma unroll
            for (int u = 0; u < K / 2; u++) {
                const u32x4 q = ldu128(vals + (cb + wrow + (uint32_t)u * 128 + (uint32_t)lane * 2) * 8);
                __builtin_memcpy(&v[2 * u], &q, 16);
            }
            uint64_t pv0 = 0;
            if (lane == 0) pv0 = ld64(vals + (cb + wrow > 0 ? cb + wrow - 1 : 0) * 8);
            uint64_t carry = readlane64(pv0, 0);
            uint32_t c = 0;  // wave-uniform: scalar adds
#pragma unroll
            for (int u = 0; u < K / 2; u++) {
                const uint64_t below = wave_shr1(v[2 * u + 1], carry);
                c += (uint32_t)__popcll(__ballot(v[2 * u] != below));
                c += (uint32_t)__popcll(__ballot(v[2 * u + 1] != v[2 * u]));
                carry = readlane64(v[2 * u + 1], 63);
            }
            if (lane == 0) changes += c;
        }
    }
    if (changes) atomicAdd(&s_total, changes);
    __syncthreads();
    if (t == 0) out[blockIdx.x] = s_total + (pad[N % PAD_WORDS] == 0xFFFFFFFFu);  // (never true: the pad stays allocated)
}

template <int LANE_ROWS>
static int run(const char* name, const uint8_t* d, uint64_t P, uint64_t N, uint32_t* out, unsigned long long* total) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) k_loads<LANE_ROWS><<<(uint32_t)P, WG>>>(d, N, out);
    CK(hipDeviceSynchronize());
    std::vector<float> ms(10);
    for (auto& m : ms) {
        CK(hipEventRecord(e0));
        k_loads<LANE_ROWS><<<(uint32_t)P, WG>>>(d, N, out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&m, e0, e1));
    }
    CK(hipGetLastError());
    std::vector<uint32_t> h(P);
    CK(hipMemcpy(h.data(), out, P * 4, hipMemcpyDeviceToHost));
    *total = 0;
    for (uint32_t x : h) *total += x;
    std::vector<float> s = ms;
    std::sort(s.begin(), s.end());
    const double med = 0.5 * (s[4] + s[5]), bytes = (double)P * N * 8;
    printf("%-44s min %.3f  median %.3f  max %.3f ms  (spread %.1f %%)  %.2f TB/s at the median  changes %llu\n   launches:", name, s[0], med,
           s[9], 100.0 * (s[9] - s[0]) / med, bytes / med / 1e9, *total);
    for (float m : ms) printf(" %.3f", m);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    const uint64_t P = (uint64_t)(argc > 1 ? atoi(argv[1]) : 8192), N = 65536;
    uint8_t* d;
    uint32_t* out;
    CK(hipMalloc(&d, P * N * 8));
    CK(hipMalloc(&out, P * 4));
    k_fill<<<(uint32_t)((P * N + 255) / 256), 256>>>((double*)d, P * N);
    CK(hipDeviceSynchronize());
    unsigned long long ta = 0, tb = 0;
    if (run<0>("(a) thread = 16 consecutive rows (64 lines)", d, P, N, out, &ta)) return 2;
    if (run<1>("(b) lane-contiguous pieces (8 lines)", d, P, N, out, &tb)) return 2;
    printf("totals %s\n", ta == tb ? "agree" : "DIFFER");
    return ta == tb ? 0 : 1;
}
