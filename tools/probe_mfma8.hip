// Probe: what csrc/attn_q8.hip assumes of the 8-bit matrix instructions of gfx950 (exit code 0 when all of it holds).
// (1) v_mfma_i32_32x32x32_i8 and v_mfma_f32_32x32x64_f8f6f4 (both operands e4m3): lane l supplies row / column (l & 31) and the l >> 5 half of the reduction
//     index, byte e of its 16 / 32 operand bytes is multiplied with byte e of the other operand's lane of the same half (so the reduction index is a dummy),
//     and the result lands in the C layout of v_mfma_f32_32x32x16_bf16: lane l holds column (l & 31), register r holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5).
// (2) v_cvt_pk_fp8_f32 writes OCP e4m3fn, round to nearest even, into the selected half-word: 448 -> 0x7e, 1 -> 0x38, 2^-9 -> 0x01, 2^-10 (a tie) -> 0x00,
//     1.5 * 2^-9 (a tie) -> 0x02, 1.0625 (a tie) -> 0x38, 1.1875 (a tie) -> 0x3a, and the sign bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// a, b: [64 lanes][32 bytes] (the int8 instruction uses the first 16 of each lane); ci / cf: [64 lanes][16 registers]
__global__ void probe_mfma(const uint8_t* a, const uint8_t* b, int* ci, float* cf) {
    const int l = threadIdx.x;
    const i32x4 a4 = *reinterpret_cast<const i32x4*>(a + l * 32), b4 = *reinterpret_cast<const i32x4*>(b + l * 32);
    i32x16 zi = {};
    const i32x16 ri = __builtin_amdgcn_mfma_i32_32x32x32_i8(a4, b4, zi, 0, 0, 0);
    const i32x8 a8 = *reinterpret_cast<const i32x8*>(a + l * 32), b8 = *reinterpret_cast<const i32x8*>(b + l * 32);
    i32x8 am, bm;
    for (int w = 0; w < 8; ++w) {  // bytes -> small e4m3 numbers: sign, exponent field 4 .. 7 (0.125 .. 1), no mantissa: every product and sum is exact
        am[w] = (a8[w] & 0x80808080) | 0x20202020 | ((a8[w] & 0x03030303) << 3);
        bm[w] = (b8[w] & 0x80808080) | 0x20202020 | ((b8[w] & 0x03030303) << 3);
    }
    f32x16 zf = {};
    const f32x16 rf = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(am, bm, zf, 0, 0, 0, 0, 0, 0);  // zero scales: the unscaled instruction
    for (int r = 0; r < 16; ++r) {
        ci[l * 16 + r] = ri[r];
        cf[l * 16 + r] = rf[r];
    }
}

// which B byte (g', e') meets A byte (g, e) in the f8f6f4 instruction: A is 1.0 at byte e of lane 32 g (row 0) alone; B column j < 6 is 1.0 where bit j of
// 32 g' + e' is set, column 6 is 1.0 everywhere.  Row 0 of the result (register 0 of lanes 0 .. 31) then spells the partner index and a presence flag.
__global__ void probe_pair(float* out) {
    const int l = threadIdx.x, j = l & 31, gb = l >> 5;
    i32x8 bm = {};
    for (int e = 0; e < 32; ++e) {
        const int k = 32 * gb + e;
        if (j == 6 || (j < 6 && ((k >> j) & 1))) bm[e >> 2] |= 0x38 << (8 * (e & 3));
    }
    for (int k = 0; k < 64; ++k) {
        i32x8 am = {};
        if (l == 32 * (k >> 5)) am[(k & 31) >> 2] = 0x38 << (8 * (k & 3));
        f32x16 zf = {};
        const f32x16 rf = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(am, bm, zf, 0, 0, 0, 0, 0, 0);
        if (l < 32) out[k * 32 + l] = rf[0];
    }
}

__global__ void probe_cvt(const float* x, uint32_t* out, int n) {
    const int i = threadIdx.x;
    if (i >= n) return;
    out[2 * i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[i], -x[i], 0x55555555, false);
    out[2 * i + 1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[i], -x[i], 0x55555555, true);
}

static float e4m3_small(uint8_t byte) {  // the value probe_mfma makes of a byte
    const float mag = 0.125f * (float)(1 << (byte & 3));
    return (byte & 0x80) ? -mag : mag;
}

int main() {
    uint8_t ha[2048], hb[2048];
    uint32_t s = 12345u;
    for (int i = 0; i < 2048; ++i) {
        s = s * 1664525u + 1013904223u;
        ha[i] = (uint8_t)(s >> 24);
        s = s * 1664525u + 1013904223u;
        hb[i] = (uint8_t)(s >> 24);
    }
    uint8_t *da, *db;
    int* dci;
    float* dcf;
    if (hipMalloc(&da, 2048) != hipSuccess || hipMalloc(&db, 2048) != hipSuccess || hipMalloc(&dci, 4096) != hipSuccess || hipMalloc(&dcf, 4096) != hipSuccess) return 2;
    (void)hipMemcpy(da, ha, 2048, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, hb, 2048, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe_mfma, dim3(1), dim3(64), 0, 0, da, db, dci, dcf);
    int hci[1024];
    float hcf[1024];
    if (hipMemcpy(hci, dci, 4096, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hcf, dcf, 4096, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad_i = 0, bad_f = 0;
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 16; ++r) {
            const int col = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            long wi = 0;
            double wf = 0;
            for (int g = 0; g < 2; ++g) {
                for (int e = 0; e < 16; ++e) wi += (long)(int8_t)ha[(g * 32 + row) * 32 + e] * (int8_t)hb[(g * 32 + col) * 32 + e];
                for (int e = 0; e < 32; ++e) wf += (double)e4m3_small(ha[(g * 32 + row) * 32 + e]) * e4m3_small(hb[(g * 32 + col) * 32 + e]);
            }
            bad_i += hci[l * 16 + r] != wi;
            if ((double)hcf[l * 16 + r] != wf && bad_f++ < 8) printf("f8f6f4: lane %d register %d: %g, want %g\n", l, r, hcf[l * 16 + r], wf);
        }
    printf("v_mfma_i32_32x32x32_i8 operand / result map: %s (%d of 1024 off)\n", bad_i ? "MISMATCH" : "MATCH", bad_i);
    printf("v_mfma_f32_32x32x64_f8f6f4 (e4m3 x e4m3) operand / result map: %s (%d of 1024 off)\n", bad_f ? "MISMATCH" : "MATCH", bad_f);

    float* dp;
    static float hp[2048];
    if (hipMalloc(&dp, sizeof(hp)) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe_pair, dim3(1), dim3(64), 0, 0, dp);
    if (hipMemcpy(hp, dp, sizeof(hp), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad_p = 0;
    printf("f8f6f4 pairing, A byte 32 g + e -> B byte (count):");
    for (int k = 0; k < 64; ++k) {
        int partner = 0;
        for (int j = 0; j < 6; ++j) partner |= (hp[k * 32 + j] != 0.f) << j;
        printf("%s%d(%g)", (k & 15) ? " " : "\n  ", partner, hp[k * 32 + 6]);
        bad_p += partner != k || hp[k * 32 + 6] != 1.f;
    }
    printf("\nf8f6f4 pairing is the identity: %s (%d of 64 off)\n", bad_p ? "NO" : "YES", bad_p);

    const float hx[8] = {448.f, 1.f, 0.001953125f, 0.0009765625f, 0.0029296875f, 1.0625f, 1.1875f, 0.f};
    const uint8_t want[8] = {0x7e, 0x38, 0x01, 0x00, 0x02, 0x38, 0x3a, 0x00};
    float* dx;
    uint32_t* dout;
    if (hipMalloc(&dx, 32) != hipSuccess || hipMalloc(&dout, 64) != hipSuccess) return 2;
    (void)hipMemcpy(dx, hx, 32, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe_cvt, dim3(1), dim3(64), 0, 0, dx, dout, 8);
    uint32_t ho[16];
    if (hipMemcpy(ho, dout, 64, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad_c = 0;
    for (int i = 0; i < 8; ++i) {
        const uint32_t pair = want[i] | ((uint32_t)(want[i] | 0x80) << 8);  // (x, -x); -0 keeps its sign bit
        const bool ok = ho[2 * i] == (0x55550000u | pair) && ho[2 * i + 1] == (0x00005555u | (pair << 16));
        if (!ok) printf("cvt: %g -> low-half form 0x%08x, high-half form 0x%08x (want bytes 0x%02x, 0x%02x)\n", hx[i], ho[2 * i], ho[2 * i + 1], want[i], want[i] | 0x80);
        bad_c += !ok;
    }
    printf("v_cvt_pk_fp8_f32 (e4m3fn, nearest even, half-word select): %s (%d of 8 off)\n", bad_c ? "MISMATCH" : "MATCH", bad_c);
    return (bad_i || bad_f || bad_p || bad_c) ? 1 : 0;
}
