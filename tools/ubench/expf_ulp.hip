// expf of the fp32 values in a file, one kernel, results to a second file: the device half of tools/expf_ulp.py, which measures
// the library function against fp64 exp on the host.  Built with the library's flags (hipcc -O3 -ffp-contract=off): the same expf
// the kernels of csrc/neigh_agg.hip call.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k(const float *__restrict__ x, float *__restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = expf(x[i]);
}
#define OK(e) do { if ((e) != hipSuccess) { fprintf(stderr, "HIP error at line %d\n", __LINE__); return 2; } } while (0)
int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: expf_ulp ARGS.f32 OUT.f32\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    std::vector<float> h(n);
    if (n == 0 || fread(h.data(), sizeof(float), n, f) != n) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    float *x, *y;
    OK(hipMalloc(&x, n * sizeof(float)));
    OK(hipMalloc(&y, n * sizeof(float)));
    OK(hipMemcpy(x, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    k<<<(unsigned)((n + 255) / 256), 256>>>(x, y, n);
    OK(hipGetLastError());
    OK(hipMemcpy(h.data(), y, n * sizeof(float), hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(h.data(), sizeof(float), n, f) != n) { perror(argv[2]); return 2; }
    fclose(f);
    return 0;
}
