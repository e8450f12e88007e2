// layer_norm.hip -- LayerNorm over fp16 rows (StarCoder2, Cohere: architecture.py:656-676, :704-721) and the bridge between two
// parallel decoder blocks (parallel_decoder.py:137-143), + their C ABI.
//
// Reference: layer_norm_cuda (layer_norm.cu:185-212) as ext_norm.cpp calls it for layer_norm / layer_norm_; numerics: layer_norm.h.
// One 256-thread workgroup per row; thread t keeps octets t + 256 k, k < K, of the row in registers between the passes: a row is
// read once (16 bytes per lane and access) and written once.  K <= LAYER_NORM_MAX_K, i.e. dim <= LAYER_NORM_MAX_DIM; any other
// shape is reported, never run on a slower path.  HBM / launch-latency bound.
#include "layer_norm.h"
#include "errors.h"

struct LayerNormArgs
{
    const f16* x; const f16* w; const f16* b; f16* y;
    float eps, r_dim;
    int dim, add_residual;
};

// y may alias x: a thread has read its octets of x (and, with add_residual, of y) before it writes them
template <int K>
KERNEL void __launch_bounds__(256) layer_norm_kernel(const LayerNormArgs a)
{
    SHARED double part1[4];
    SHARED double part2[4];
    const int t = tid();
    const int dim8 = a.dim >> 3;          // host guarantees dim % 8 == 0 and dim8 <= 256 K
    const size_t row0 = (size_t)bid_x() * a.dim;

    const f16x8* xr = (const f16x8*)(a.x + row0);
    float f[K][8];
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8) layer_norm_widen(xr[i], f[k]);
        else
        {
            #pragma unroll
            for (int e = 0; e < 8; e++) f[k][e] = 0.0f;
        }
    }
    const float rsvar = layer_norm_centre<K>(f, dim8, a.r_dim, a.eps, part1, part2);

    const f16x8* wr = (const f16x8*)a.w;
    const f16x8* br = (const f16x8*)a.b;
    f16x8* yr = (f16x8*)(a.y + row0);
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            f16x8 o = layer_norm_scale(f[k], wr[i], rsvar);
            if (br) o = o + br[i];                       // __hadd2(nh, b) (layer_norm.cu:152)
            if (a.add_residual) o = o + yr[i];           // __hadd2(nh, y) (layer_norm.cu:155)
            yr[i] = o;
        }
    }
}

// ---- parallel bridge ----------------------------------------------------------------------------------------------------
// The tail of a parallel block and the head of the next, in one launch:
//   x += a; x += b           two fp16 adds in that order (parallel_decoder.py:141-142), a / b null: x is read only
//   n0 = n1 = LN(x) * w + bias   the next block's input_layernorm (or the final norm) through layer_norm.h: bit for bit what
//                            exl2_layer_norm gives on the new x; n1 null: one copy; w null: the adds only
// n0 may alias a and n1 may alias b (the attention and the MLP of a parallel block run in place on the two normed copies): a thread
// has read its octets of a and b before it writes them.  x is read once, written once and never re-read.
struct ParallelBridgeArgs
{
    f16* x; const f16* a; const f16* b; const f16* w; const f16* bias; f16* n0; f16* n1;
    float eps, r_dim;
    int dim;
};

template <int K>
KERNEL void __launch_bounds__(256) parallel_bridge_kernel(const ParallelBridgeArgs p)
{
    SHARED double part1[4];
    SHARED double part2[4];
    const int t = tid();
    const int dim8 = p.dim >> 3;
    const size_t row0 = (size_t)bid_x() * p.dim;

    f16x8* xr = (f16x8*)(p.x + row0);
    const f16x8* ar = (const f16x8*)(p.a + row0);
    const f16x8* br = (const f16x8*)(p.b + row0);
    float f[K][8];
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            f16x8 v = xr[i];
            if (p.a)                                     // (a and b come together: host)
            {
                v = v + ar[i];
                v = v + br[i];
                xr[i] = v;
            }
            layer_norm_widen(v, f[k]);
        }
        else
        {
            #pragma unroll
            for (int e = 0; e < 8; e++) f[k][e] = 0.0f;
        }
    }
    if (!p.w) return;                                    // (uniform over the launch)
    const float rsvar = layer_norm_centre<K>(f, dim8, p.r_dim, p.eps, part1, part2);

    const f16x8* wr = (const f16x8*)p.w;
    const f16x8* biasr = (const f16x8*)p.bias;
    f16x8* n0r = (f16x8*)(p.n0 + row0);
    f16x8* n1r = (f16x8*)(p.n1 + row0);
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            f16x8 o = layer_norm_scale(f[k], wr[i], rsvar);
            if (biasr) o = o + biasr[i];
            n0r[i] = o;
            if (p.n1) n1r[i] = o;
        }
    }
}

// x += a over numel elements (numel % 8 == 0), one fp16 add each: the adds of a parallel block where the bridge is not taken
KERNEL void __launch_bounds__(256) add_f16_kernel(f16* x, const f16* a, long long nvec)
{
    const long long i = (long long)bid_x() * 256 + tid();
    if (i < nvec) ((f16x8*)x)[i] = ((const f16x8*)x)[i] + ((const f16x8*)a)[i];
}

// the instantiation for K octets per thread: 1, 2, 3, 4, 6 or 8 (5 runs as 6, 7 as 8: the surplus octets are beyond dim8)
#define LAYER_NORM_DISPATCH(kernel, k, rows, stream, args)                                              \
    do {                                                                                                \
        if ((k) <= 1)      LAUNCH(kernel<1>, dim3((unsigned)(rows)), dim3(256), 0, stream, args);       \
        else if ((k) == 2) LAUNCH(kernel<2>, dim3((unsigned)(rows)), dim3(256), 0, stream, args);       \
        else if ((k) == 3) LAUNCH(kernel<3>, dim3((unsigned)(rows)), dim3(256), 0, stream, args);       \
        else if ((k) == 4) LAUNCH(kernel<4>, dim3((unsigned)(rows)), dim3(256), 0, stream, args);       \
        else if ((k) <= 6) LAUNCH(kernel<6>, dim3((unsigned)(rows)), dim3(256), 0, stream, args);       \
        else               LAUNCH(kernel<LAYER_NORM_MAX_K>, dim3((unsigned)(rows)), dim3(256), 0, stream, args); \
    } while (0)

static bool ln_aligned16(const void* p) { return (((size_t)p) & 15) == 0; }
static bool ln_covered(int dim) { return dim > 0 && dim % 8 == 0 && dim <= LAYER_NORM_MAX_DIM; }

extern "C" {

// layer_norm / layer_norm_ (ext_norm.cpp -> layer_norm_cuda): y = LN(x) * w (+ b) (+ old y); b nullable; y == x: in place
int exl2_layer_norm(const void* x, const void* w, const void* b, void* y, float epsilon, int rows, int dim, int add_residual,
                    void* stream)
{
    EXL2_REQUIRE(x && w && y, "layer_norm: null argument");
    if (!ln_covered(dim))
        EXL2_FAIL(EXL2_E_UNSUPPORTED, "layer_norm: shape not covered: dim %d must be a multiple of 8 up to %d", dim, LAYER_NORM_MAX_DIM);
    EXL2_REQUIRE(ln_aligned16(x) && ln_aligned16(w) && ln_aligned16(b) && ln_aligned16(y), "layer_norm: x / w / b / y must be 16-byte aligned");
    if (rows <= 0) return EXL2_OK;
    LayerNormArgs a;
    a.x = (const f16*)x; a.w = (const f16*)w; a.b = (const f16*)b; a.y = (f16*)y;
    a.eps = epsilon; a.r_dim = 1.0f / (float)dim; a.dim = dim; a.add_residual = add_residual ? 1 : 0;
    const int k = ((dim >> 3) + 255) / 256;
    LAYER_NORM_DISPATCH(layer_norm_kernel, k, rows, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

// returns 0 when launched, 1 when the shape is not covered (dim no multiple of 8 or above LAYER_NORM_MAX_DIM): nothing was launched,
// nothing is touched -- the caller runs exl2_add_f16 twice and exl2_layer_norm
int exl2_parallel_bridge(void* x, const void* a, const void* b, const void* w, const void* bias, void* n0, void* n1, float epsilon,
                         int rows, int dim, void* stream)
{
    EXL2_REQUIRE(x, "parallel_bridge: null argument");
    EXL2_REQUIRE((a != nullptr) == (b != nullptr), "parallel_bridge: a and b come together");
    EXL2_REQUIRE(a || w, "parallel_bridge: nothing to do (no a / b and no w)");
    EXL2_REQUIRE(!w || n0, "parallel_bridge: w needs n0");
    EXL2_REQUIRE(w || !bias, "parallel_bridge: bias without w");
    EXL2_REQUIRE(dim > 0, "parallel_bridge: dim %d", dim);
    if (!ln_covered(dim)) return 1;
    EXL2_REQUIRE(ln_aligned16(x) && ln_aligned16(a) && ln_aligned16(b) && ln_aligned16(w) && ln_aligned16(bias) && ln_aligned16(n0) && ln_aligned16(n1),
                 "parallel_bridge: x / a / b / w / bias / n0 / n1 must be 16-byte aligned");
    if (rows <= 0) return EXL2_OK;
    ParallelBridgeArgs p;
    p.x = (f16*)x; p.a = (const f16*)a; p.b = (const f16*)b; p.w = (const f16*)w; p.bias = (const f16*)bias;
    p.n0 = (f16*)n0; p.n1 = w ? (f16*)n1 : nullptr;
    p.eps = epsilon; p.r_dim = 1.0f / (float)dim; p.dim = dim;
    const int k = ((dim >> 3) + 255) / 256;
    LAYER_NORM_DISPATCH(parallel_bridge_kernel, k, rows, stream, p);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

int exl2_add_f16(void* x, const void* a, long long numel, void* stream)
{
    EXL2_REQUIRE(x && a, "add_f16: null argument");
    EXL2_REQUIRE(numel >= 0 && numel % 8 == 0, "add_f16: %lld elements are no multiple of 8", numel);
    EXL2_REQUIRE(ln_aligned16(x) && ln_aligned16(a), "add_f16: x / a must be 16-byte aligned");
    if (numel == 0) return EXL2_OK;
    const long long nvec = numel / 8, blocks = (nvec + 255) / 256;
    EXL2_REQUIRE(blocks <= 0x7fffffffLL, "add_f16: %lld elements exceed one launch", numel);
    LAUNCH(add_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (f16*)x, (const f16*)a, nvec);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

}  // extern "C"
