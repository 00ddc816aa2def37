// Where does the per-output-tile cost `a` of gemm_nt8 (time per tile = a + b * K/64) go?
//
//   hipcc --offload-arch=gfx950 -O3 -I include tests/probes/gemm_tile_probe.hip -L commu-code_amd/lib -lcommu_hip \
//         -Wl,-rpath,$PWD/commu-code_amd/lib -o tests/probes/bin/gemm_tile_probe
//   tests/probes/bin/gemm_tile_probe > profiles/<name>.txt
//
// 1. times commu_gemm_nt_bf16 at the isolated NT shapes of the training step (M = 65536) in the forms the step launches
//    (pipelined plain / bias+relu+dropout epilogue, burst epilogue with a residual) and refits a and b;
// 2. the same shapes with the profiling builds ABL 3 (no epilogue) and ABL 2 (no staging), on half the CUs
//    (COMMU_GEMM8_GRID=128) and with a start-up skew of one tile time over the eight classes (COMMU_GEMM8_SKEW);
// 3. ABL 4: wave 0 of every workgroup stamps the shader clock after each of the eight barriers of a K-tile; printed are the
//    medians over the workgroups of every barrier-to-barrier interval of the first 32 K-tiles of a workgroup's stream: a tile's
//    last K-tile and the next tile's first ones against the same intervals in mid-tile.  (Intervals only: the clocks of
//    different XCDs are not synchronised, so stamps of different workgroups cannot be compared.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "commu_hip.h"

extern "C" void commu_gemm8_probe(int abl, void* stamps);

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

__global__ void fill_bf16(unsigned short* p, size_t n, unsigned seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const float v = ((int)(h & 0xFFFF) - 32768) * (scale / 32768.f);
        p[i] = (unsigned short)(__float_as_uint(v) >> 16);
    }
}
__global__ void fill_f32(float* p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v + 1e-3f * (i & 7);
}

static const int M = 65536;
static void *A, *B, *C, *R;
static float* bias;
static hipEvent_t e0, e1;

enum Form { PLAIN, BRD, RESID };          // plain, bias + relu + dropout (both pipelined), residual + dropout (burst)
static int launch(int N, int K, Form f) {
    const int flags = f == PLAIN ? 0 : f == BRD ? (COMMU_EPI_BIAS | COMMU_EPI_RELU | COMMU_EPI_DROPOUT) : (COMMU_EPI_RESID | COMMU_EPI_DROPOUT);
    return commu_gemm_nt_bf16(A, K, B, K, C, N, M, N, K, f == BRD ? bias : nullptr, f == RESID ? R : nullptr, N, nullptr, 0, flags,
                              1234u, f == PLAIN ? 0.f : 0.1f, 1.f, 0);
}
static float time_us(int N, int K, Form f, int iters = 20) {
    for (int i = 0; i < 3; ++i)
        if (launch(N, K, f) != 0) { fprintf(stderr, "launch failed\n"); exit(1); }
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) launch(N, K, f);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1000.f / iters;
}
static void fit(const std::vector<double>& x, const std::vector<double>& y, double& a, double& b) {
    double sx = 0, sy = 0, sxx = 0, sxy = 0;
    const int n = (int)x.size();
    for (int i = 0; i < n; ++i) { sx += x[i]; sy += y[i]; sxx += x[i] * x[i]; sxy += x[i] * y[i]; }
    b = (n * sxy - sx * sy) / (n * sxx - sx * sx);
    a = (sy - b * sx) / n;
}
static double median(std::vector<double> v) {
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main() {
    const int shapes[][2] = {{512, 512}, {512, 1024}, {512, 1536}, {1024, 512}, {1536, 512}, {512, 2048}, {1536, 2048}};
    const int nshapes = sizeof(shapes) / sizeof(shapes[0]);
    const int Kmax = 2048, Nmax = 1536;
    CK(hipMalloc(&A, (size_t)M * Kmax * 2));
    CK(hipMalloc(&B, (size_t)Nmax * Kmax * 2));
    CK(hipMalloc(&C, (size_t)M * Nmax * 2));
    CK(hipMalloc(&R, (size_t)M * Nmax * 2));
    CK(hipMalloc(&bias, Nmax * 4));
    unsigned* stamps;
    const int SW = 256;          // stamps per workgroup: 32 K-tiles x 8 barriers
    CK(hipMalloc(&stamps, 256 * SW * 4));
    hipLaunchKernelGGL(fill_bf16, dim3(2048), dim3(256), 0, 0, (unsigned short*)A, (size_t)M * Kmax, 1u, 1.f);
    hipLaunchKernelGGL(fill_bf16, dim3(2048), dim3(256), 0, 0, (unsigned short*)B, (size_t)Nmax * Kmax, 2u, 0.05f);
    hipLaunchKernelGGL(fill_bf16, dim3(2048), dim3(256), 0, 0, (unsigned short*)R, (size_t)M * Nmax, 3u, 1.f);
    hipLaunchKernelGGL(fill_f32, dim3(8), dim3(256), 0, 0, bias, (size_t)Nmax, 0.01f);
    CK(hipDeviceSynchronize());
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    // clocks up before the first number
    for (int i = 0; i < 200; ++i) launch(1536, 2048, PLAIN);
    CK(hipDeviceSynchronize());

    struct Var { const char* name; Form f; int abl; const char* grid; int skew8; bool nopipe; };
    // skew8: COMMU_GEMM8_SKEW = (that shape's plain tile time in shader cycles at 2.4 GHz) / 8 when set
    const Var vars[] = {
        {"plain", PLAIN, 0, nullptr, 0, false},      {"bias+relu+drop", BRD, 0, nullptr, 0, false},
        {"resid+drop(burst)", RESID, 0, nullptr, 0, false}, {"plain burst", PLAIN, 0, nullptr, 0, true},
        {"plain ABL3", PLAIN, 3, nullptr, 0, false}, {"plain ABL2", PLAIN, 2, nullptr, 0, false},
        {"plain grid128", PLAIN, 0, "128", 0, false}, {"ABL3 grid128", PLAIN, 3, "128", 0, false},
        {"resid grid128", RESID, 0, "128", 0, false}, {"plain skew", PLAIN, 0, nullptr, 1, false},
        {"plain ABL4(stamps)", PLAIN, 4, nullptr, 0, false}, {"plain again", PLAIN, 0, nullptr, 0, false},
    };
    const int nvars = sizeof(vars) / sizeof(vars[0]);
    std::vector<std::vector<double>> per_tile(nvars, std::vector<double>(nshapes));
    printf("# gemm_nt8, M = %d, time per launch in us (20 launches back to back); tiles per workgroup = N/256 (grid 128: 2N/256)\n", M);
    printf("%-22s", "N x K");
    for (int s = 0; s < nshapes; ++s) printf(" %5dx%-5d", shapes[s][0], shapes[s][1]);
    printf("\n");
    for (int v = 0; v < nvars; ++v) {
        printf("%-22s", vars[v].name);
        for (int s = 0; s < nshapes; ++s) {
            const int N = shapes[s][0], K = shapes[s][1];
            commu_gemm8_probe(vars[v].abl, vars[v].abl == 4 ? (void*)stamps : nullptr);
            if (vars[v].grid) setenv("COMMU_GEMM8_GRID", vars[v].grid, 1); else unsetenv("COMMU_GEMM8_GRID");
            if (vars[v].nopipe) setenv("COMMU_GEMM8_NOPIPE", "1", 1); else unsetenv("COMMU_GEMM8_NOPIPE");
            if (vars[v].skew8) {
                char buf[32];
                snprintf(buf, sizeof buf, "%d", (int)(per_tile[0][s] * 2400.0 / 8));
                setenv("COMMU_GEMM8_SKEW", buf, 1);
            } else unsetenv("COMMU_GEMM8_SKEW");
            const float us = time_us(N, K, vars[v].f);
            const int tpw = (N / 256) * (vars[v].grid ? 2 : 1);
            per_tile[v][s] = us / tpw;
            printf(" %11.1f", us);
        }
        printf("\n");
        fflush(stdout);
    }
    commu_gemm8_probe(0, nullptr);
    unsetenv("COMMU_GEMM8_GRID"); unsetenv("COMMU_GEMM8_NOPIPE"); unsetenv("COMMU_GEMM8_SKEW");
    printf("\n# fit: time per tile = a + b * (K/64), least squares over the %d shapes (us)\n", nshapes);
    for (int v = 0; v < nvars; ++v) {
        std::vector<double> x(nshapes);
        for (int s = 0; s < nshapes; ++s) x[s] = shapes[s][1] / 64;
        double a, b;
        fit(x, per_tile[v], a, b);
        printf("%-22s a = %6.2f  b = %6.3f   a alone at", vars[v].name, a, b);
        for (int s = 0; s < nshapes; ++s) printf(" %5.1f", per_tile[v][s] - b * x[s]);
        printf("\n");
    }

    // ---- stamps
    const int st_shapes[][2] = {{512, 512}, {1536, 512}, {1024, 512}, {512, 1536}};
    for (int f = 0; f < 3; ++f)
    for (int s = 0; s < 4; ++s) {
        const int N = st_shapes[s][0], K = st_shapes[s][1], nk = K / 64, tpw = N / 256;
        if (f > 0 && s > 1) continue;
        commu_gemm8_probe(4, stamps);
        for (int i = 0; i < 5; ++i) launch(N, K, (Form)f);
        CK(hipDeviceSynchronize());
        std::vector<unsigned> h(256 * SW);
        CK(hipMemcpy(h.data(), stamps, h.size() * 4, hipMemcpyDeviceToHost));
        commu_gemm8_probe(0, nullptr);
        const int nkt = std::min(32, nk * tpw);
        printf("\n# ABL 4, form %s, N = %d, K = %d (nk = %d, %d tiles per workgroup): median over 256 workgroups of the shader cycles between\n"
               "# consecutive barriers of wave 0 (b0: phase 1 loads+drain -> b1: MFMAs -> b2: phase 2 loads -> ... b7); '*' = first K-tile of a tile\n",
               f == 0 ? "plain" : f == 1 ? "bias+relu+drop" : "resid+drop(burst)", N, K, nk, tpw);
        printf("%4s %8s %8s %8s %8s %8s %8s %8s %8s %9s\n", "kt", "->b0", "->b1", "->b2", "->b3", "->b4", "->b5", "->b6(w)", "->b7", "K-tile");
        for (int kt = 0; kt < nkt; ++kt) {
            printf("%3d%c", kt, kt % nk == 0 ? '*' : ' ');
            double tot = 0;
            for (int k = 0; k < 8; ++k) {
                std::vector<double> d;
                for (int wg = 0; wg < 256; ++wg) {
                    const int i = kt * 8 + k;
                    if (i == 0) continue;
                    const unsigned t1 = h[wg * SW + i], t0 = h[wg * SW + i - 1];
                    if (t1 && t0) d.push_back((double)(unsigned)(t1 - t0));
                }
                const double m = median(d);
                tot += m;
                printf(" %8.0f", m);
            }
            printf(" %9.0f\n", tot);
        }
    }
    return 0;
}
