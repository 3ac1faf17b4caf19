// mfma16_layout_probe.hip — the operand and accumulator layout of v_mfma_f32_16x16x32_f16 by experiment (one launch of one wavefront),
// the layout k_lstm2_w16 and its packing (pack_lstm2_w16, pack_l4_w16) rely on:
//   A: lane l holds A[row l % 16][k = 8 (l / 16) + e], e = 0..7     B: lane l holds B[k = 8 (l / 16) + e][col l % 16]
//   D: lane l holds D[row 4 (l / 16) + j][col l % 16], j = 0..3
// Three products with exact small integers: A = [I | 0] (D = the top 16 rows of B), B = [I ; 0] (D = the left 16 columns of A), and
// pseudo-random integers in both operands over all 32 k.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/mfma16_layout_probe.hip -o tools/mfma16_layout_probe
#include <hip/hip_runtime.h>
#include <cstdio>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

__global__ void k_probe(const _Float16 *a, const _Float16 *b, float *d) {      // a, b: [64 lanes][8]; d: [64 lanes][4]
    const int l = threadIdx.x;
    half8 va, vb;
    for (int e = 0; e < 8; ++e) { va[e] = a[l * 8 + e]; vb[e] = b[l * 8 + e]; }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, vb, acc, 0, 0, 0);
    for (int j = 0; j < 4; ++j) d[l * 4 + j] = acc[j];
}

static int run(const float (*A)[32], const float (*B)[16], const char *name) {
    _Float16 ha[512], hb[512];
    for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
            ha[l * 8 + e] = (_Float16)A[l % 16][8 * (l / 16) + e];
            hb[l * 8 + e] = (_Float16)B[8 * (l / 16) + e][l % 16];
        }
    _Float16 *da, *db; float *dd, hd[256];
    if (hipMalloc(&da, sizeof ha) || hipMalloc(&db, sizeof hb) || hipMalloc(&dd, sizeof hd)) { printf("hipMalloc failed\n"); return 1; }
    (void)hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, da, db, dd);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    (void)hipMemcpy(hd, dd, sizeof hd, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 4; ++j) {
            const int r = 4 * (l / 16) + j, c = l % 16;
            float want = 0.f;
            for (int k = 0; k < 32; ++k) want += A[r][k] * B[k][c];
            if (hd[l * 4 + j] != want && bad++ < 8) printf("%s: lane %d reg %d = %g, want D[%d][%d] = %g\n", name, l, j, hd[l * 4 + j], r, c, want);
        }
    printf("%s: %s\n", name, bad ? "MISMATCH" : "layout as assumed");
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dd);
    return bad != 0;
}

int main() {
    static float A[16][32], B[32][16];
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 32; ++k) A[r][k] = (k == r) ? 1.f : 0.f;
    for (int k = 0; k < 32; ++k) for (int c = 0; c < 16; ++c) B[k][c] = (float)(k * 16 + c);
    int rc = run(A, B, "A = [I | 0]");
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 32; ++k) A[r][k] = (float)(r * 32 + k);
    for (int k = 0; k < 32; ++k) for (int c = 0; c < 16; ++c) B[k][c] = (k == c) ? 1.f : 0.f;
    rc |= run(A, B, "B = [I ; 0]");
    unsigned x = 12345;                                      // all of K: small pseudo-random integers in both operands (exact sums)
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 32; ++k) { x = x * 1103515245u + 12345u; A[r][k] = (float)((int)((x >> 16) % 15) - 7); }
    for (int k = 0; k < 32; ++k) for (int c = 0; c < 16; ++c) { x = x * 1103515245u + 12345u; B[k][c] = (float)((int)((x >> 16) % 15) - 7); }
    rc |= run(A, B, "random");
    return rc;
}
