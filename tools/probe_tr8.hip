// Probe: (1) the lane / element map of ds_read_b64_tr_b8 on gfx950, against the map csrc/gemm_w8.hip is written for; (2) v_cvt_scalef32_pk_bf16_fp8 at
// scale 1.0 on all 256 e4m3fn bytes in all four byte positions, against the bit arithmetic of csrc/cast.hip.
// LDS byte a holds a (low byte in pass 0, high byte in pass 1); lane l supplies the address 8 l.  Expected: inside each 16-lane group, lane 2 j + q supplies
// R[j][8 q .. 8 q + 7] of an 8 x 16 byte matrix R and lane c receives column c: (R[0][c], ..., R[7][c]) -- i.e. lane 16 u + c gets bytes 128 u + c + 16 {0..7}.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__global__ void probe_tr(uint8_t* out, int pass) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[512];
    for (int i = threadIdx.x; i < 512; i += 64) lds[i] = (uint8_t)(pass ? i >> 8 : i);
    __syncthreads();
    const i32x2 r = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(lds + threadIdx.x * 8));
    for (int e = 0; e < 8; ++e) out[threadIdx.x * 8 + e] = (uint8_t)((unsigned)r[e >> 2] >> (8 * (e & 3)));
}

__global__ void probe_cvt(uint16_t* out) {  // out[(pos * 256 + byte)] = the bf16 the instruction makes of `byte` at byte position `pos` of the source word
    const unsigned b = threadIdx.x;
    for (int pos = 0; pos < 4; ++pos) {
        const unsigned word = (b << (8 * pos)) | (0x38383838u & ~(0xffu << (8 * pos)));  // the other three bytes: 1.0
        const bf16x2_t v = (pos & 2) ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, false);
        const unsigned bits = __builtin_bit_cast(unsigned, v);
        out[pos * 256 + b] = (uint16_t)((pos & 1) ? bits >> 16 : bits & 0xffff);
        out[1024 + pos * 256 + b] = (uint16_t)((pos & 1) ? bits & 0xffff : bits >> 16);  // the neighbour, which must be 1.0 = 0x3f80
    }
}

static uint16_t ref_bf16(unsigned b) {
    const unsigned s = (b & 0x80u) << 8, e = (b >> 3) & 15u, m = b & 7u;
    if (e == 0) {
        const float f = (float)m * 0.001953125f;
        unsigned u;
        __builtin_memcpy(&u, &f, 4);
        return (uint16_t)(s | (u >> 16));
    }
    if ((b & 0x7fu) == 0x7fu) return (uint16_t)(s | 0x7fc0u);
    return (uint16_t)(s | ((e + 120u) << 7) | (m << 4));
}

int main() {
    uint8_t* d;
    if (hipMalloc(&d, 4096) != hipSuccess) return 2;
    uint8_t lo[512], hi[512];
    hipLaunchKernelGGL(probe_tr, dim3(1), dim3(64), 0, 0, d, 0);
    if (hipMemcpy(lo, d, 512, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe_tr, dim3(1), dim3(64), 0, 0, d, 1);
    if (hipMemcpy(hi, d, 512, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    for (int l = 0; l < 64; ++l) {
        printf("lane %2d:", l);
        for (int e = 0; e < 8; ++e) {
            const int got = hi[l * 8 + e] * 256 + lo[l * 8 + e], want = 128 * (l >> 4) + (l & 15) + 16 * e;
            bad += got != want;
            printf(" %3d", got);
        }
        printf("\n");
    }
    printf("ds_read_b64_tr_b8 lane map: %s (%d elements off)\n", bad ? "MISMATCH" : "MATCH", bad);

    uint16_t h[2048];
    hipLaunchKernelGGL(probe_cvt, dim3(1), dim3(256), 0, 0, (uint16_t*)d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int cbad = 0;
    for (int pos = 0; pos < 4; ++pos)
        for (unsigned b = 0; b < 256; ++b) {
            const uint16_t got = h[pos * 256 + b], want = ref_bf16(b);
            const bool nan_byte = (b & 0x7f) == 0x7f, got_nan = (got & 0x7f80) == 0x7f80 && (got & 0x7f);
            const bool ok = (nan_byte ? got_nan : got == want) && h[1024 + pos * 256 + b] == 0x3f80;
            if (!ok) {
                if (cbad < 40) printf("cvt: byte 0x%02x at position %d -> 0x%04x (want 0x%04x), neighbour 0x%04x\n", b, pos, got, want, h[1024 + pos * 256 + b]);
                ++cbad;
            }
        }
    printf("v_cvt_scalef32_pk_bf16_fp8 at scale 1.0: %s (%d of 1024 off)\n", cbad ? "MISMATCH" : "MATCH", cbad);
    return (bad || cbad) ? 1 : 0;
}
