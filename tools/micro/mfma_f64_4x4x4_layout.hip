// mfma_f64_4x4x4_layout.hip -- where v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 blocks per instruction, one double
// per lane for A, B and the accumulator) keeps its operands on gfx950. One wave per pair (la, lb): A is 1 in lane la alone,
// B is 1 in lane lb alone, and the wave reports which lanes of D are not zero. Printed: for every block, the 16 x 16 table
// "D lane of (A lane, B lane)" (-1: the two do not meet), then the same with the A-broadcast cbsz = 2, abid = 1 (block 1's
// A lanes feed all four blocks). Last, the SHARED-A, 16-column use of the direct solver's eight-row tile (bcr.hip, BcrAop): the
// same 4 x 4 matrix A in all four blocks, a = A[lane % 4][lane / 16], against a 4 x 16 matrix X held as the 16x16x4
// B-operand, b = X[lane / 16][lane % 16]; the product A X is expected in lane 16 i + c for entry (i, c) -- register g of a
// 16x16x4 accumulator tile when A is row group g of a row tile. Integer entries: the comparison is for equality.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_f64_4x4x4_layout.hip -o build/micro/mfma_f64_4x4x4_layout
#include <hip/hip_runtime.h>
#include <cstdio>
template <int CBSZ, int ABID>
__global__ __launch_bounds__(64) void k(unsigned long long *mask) {
    const int la = blockIdx.x >> 6, lb = blockIdx.x & 63, lane = threadIdx.x;
    const double a = lane == la ? 1.0 : 0.0, b = lane == lb ? 1.0 : 0.0;
    const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, CBSZ, ABID, 0);
    const unsigned long long m = __ballot(d != 0.0);
    if (lane == 0) mask[blockIdx.x] = m;
}
__global__ __launch_bounds__(64) void k_shared_a(const double *A, const double *X, double *D) {
    const int lane = threadIdx.x;
    D[lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(A[(lane & 3) * 4 + (lane >> 4)], X[(lane >> 4) * 16 + (lane & 15)], 0.0, 0, 0, 0);
}
static void show(const char *what, const unsigned long long *h) {
    printf("== %s\n", what);
    int cross = 0, multi = 0;
    for (int la = 0; la < 64; la++)
        for (int lb = 0; lb < 64; lb++) {
            const unsigned long long m = h[la * 64 + lb];
            if (m && (m & (m - 1))) multi++;
            if (m && (la >> 4) != (lb >> 4)) cross++;
        }
    printf("pairs with more than one D lane: %d, pairs across blocks: %d\n", multi, cross);
    for (int blk = 0; blk < 4; blk++) {
        printf("block %d: rows = A lane %d.., columns = B lane %d..\n", blk, 16 * blk, 16 * blk);
        for (int la = 16 * blk; la < 16 * blk + 16; la++) {
            for (int lb = 16 * blk; lb < 16 * blk + 16; lb++) {
                const unsigned long long m = h[la * 64 + lb];
                printf(" %3d", m ? __builtin_ctzll(m) : -1);
            }
            printf("\n");
        }
    }
}
int main() {
    unsigned long long *mask, h[4096];
    if (hipMalloc(&mask, sizeof(h)) != hipSuccess) return 1;
    k<0, 0><<<4096, 64>>>(mask);
    if (hipMemcpy(h, mask, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    show("cbsz 0", h);
    k<2, 1><<<4096, 64>>>(mask);
    if (hipMemcpy(h, mask, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("== cbsz 2, abid 1: D lanes (as a mask) of A lane 16 + r against B lane c, first 16 B lanes of every block\n");
    for (int la = 16; la < 32; la++) {
        for (int blk = 0; blk < 4; blk++) {
            for (int lb = 16 * blk; lb < 16 * blk + 16; lb++) {
                const unsigned long long m = h[la * 64 + lb];
                printf(" %2d", m ? __builtin_ctzll(m) : -1);
            }
            printf(" |");
        }
        printf("\n");
    }
    int other = 0;
    for (int la = 0; la < 64; la++)
        if ((la >> 4) != 1)
            for (int lb = 0; lb < 64; lb++) other += h[la * 64 + lb] != 0;
    printf("A lanes outside block 1 that reach D: %d\n", other);
    double hA[16], hX[64], hD[64], *dA, *dX, *dD;
    for (int e = 0; e < 16; e++) hA[e] = 1 + e;            // A[i][k] = 1 + 4 i + k
    for (int e = 0; e < 64; e++) hX[e] = 100 + 7 * e;      // X[k][c] = 100 + 7 (16 k + c)
    if (hipMalloc(&dA, sizeof(hA)) != hipSuccess || hipMalloc(&dX, sizeof(hX)) != hipSuccess ||
        hipMalloc(&dD, sizeof(hD)) != hipSuccess)
        return 1;
    if (hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice) != hipSuccess) return 1;
    if (hipMemcpy(dX, hX, sizeof(hX), hipMemcpyHostToDevice) != hipSuccess) return 1;
    k_shared_a<<<1, 64>>>(dA, dX, dD);
    if (hipMemcpy(hD, dD, sizeof(hD), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("== shared A, sixteen columns: lane 16 i + c (row i of the table, column c) against (A X)[i][c]\n");
    int wrong = 0;
    for (int i = 0; i < 4; i++) {
        for (int c = 0; c < 16; c++) {
            double want = 0.0;
            for (int kk = 0; kk < 4; kk++) want += hA[i * 4 + kk] * hX[kk * 16 + c];
            wrong += hD[16 * i + c] != want;
            printf(" %6.0f%c", hD[16 * i + c], hD[16 * i + c] == want ? ' ' : '!');
        }
        printf("\n");
    }
    printf("entries that differ from A X: %d\n", wrong);
    return 0;
}
