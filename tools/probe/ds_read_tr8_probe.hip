// Probe: lane mapping of ds_read_b64_tr_b8 on gfx950.  Every lane supplies the address of its own 8 bytes (lane l -> LDS
// bytes 8l .. 8l+7); the LDS holds each byte's own offset (two passes: low and high byte of the offset), so the result
// names the (lane, byte) every returned byte came from.  Prints the map of the first 16 lanes and checks the reading
// attention_fp8kv.hip relies on:
//   inside each block of 16 lanes the 16 x 8 bytes form an 8-row x 16-column byte matrix (lane i = row i >> 1, columns
//   8 (i & 1) .. + 7), and lane i receives column i: result byte j of lane i = byte (i & 7) of lane 2 j + (i >> 3).
// Build: hipcc --offload-arch=gfx950 -O2 tools/probe/ds_read_tr8_probe.hip -o tools/probe/ds_read_tr8_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((address_space(3))) i32x2* lds_i32x2_ptr;

__global__ void k(unsigned char* out) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[512];
    const int lane = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = lane; i < 512; i += 64) lds[i] = pass ? (unsigned char)(i >> 8) : (unsigned char)(i & 255);
        __syncthreads();
        const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2_ptr)(lds + lane * 8));
        __syncthreads();
        for (int j = 0; j < 8; ++j) out[(pass * 64 + lane) * 8 + j] = (unsigned char)((unsigned)v[j >> 2] >> (8 * (j & 3)));
    }
}

int main() {
    unsigned char *d, h[1024];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    for (int lane = 0; lane < 64; ++lane) {
        if (lane < 16) printf("lane %2d <-", lane);
        for (int j = 0; j < 8; ++j) {
            const int off = h[lane * 8 + j] | (h[(64 + lane) * 8 + j] << 8);
            const int i = lane & 15, want = ((lane & ~15) + 2 * j + (i >> 3)) * 8 + (i & 7);
            if (lane < 16) printf("  (lane %2d, byte %d)", off >> 3, off & 7);
            bad += off != want;
        }
        if (lane < 16) printf("\n");
    }
    printf("mismatches against the 8 x 16 block-transpose reading: %d of 512\n", bad);
    return bad ? 1 : 0;
}
