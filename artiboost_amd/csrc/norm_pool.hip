// HBM-bound NHWC elementwise / reduction kernels around the conv stack: training-mode BatchNorm (statistics, apply,
// backward), ReLU and residual fusion, 3x3/2 max-pool, global average pool, precision packing.
// All tensors are [M = N*H*W pixels][C channels] with C % 8 == 0; every access is a 16-byte vector per lane.
//
// Every arithmetic body of the family is written ONCE below ("shared bodies") and the __global__ kernels only choose the loads, the
// stores and the thread mapping around it: for this file the bits are the contract (the folded conv epilogues must agree with
// bn_apply, every backward mask with the forward expression), and a copy that drifts by one operation is a silent wrong gradient.
#include "common.h"
#include <type_traits>

template <typename T> struct Vec;
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };

// ================================================================ shared bodies: vector access
// N 32-bit words at p in one 4-, 8- or 16-byte access
template <int N> __device__ __forceinline__ void ld_words(const void* p, uint32_t* w) {
    if constexpr (N == 4) { const uint4 v = *(const uint4*)p; w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else if constexpr (N == 2) { const uint2 v = *(const uint2*)p; w[0] = v.x; w[1] = v.y; }
    else w[0] = *(const uint32_t*)p;
}
template <int N> __device__ __forceinline__ void st_words(void* p, const uint32_t* w) {
    if constexpr (N == 4) *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
    else if constexpr (N == 2) *(uint2*)p = make_uint2(w[0], w[1]);
    else *(uint32_t*)p = w[0];
}
// V elements at p widened to fp32 (V = 4 or 8; fp32: 16-byte vectors).  T = bf16_t is also the decode of ONE plane of a split
// tensor -- the hi plane alone carries the sign, which is all a ReLU mask needs of the activation.
template <typename T, int V = Vec<T>::N> __device__ __forceinline__ void vload(const T* p, float* f) {
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            const float4 v = *(const float4*)(p + 4 * i);
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
    } else {
        uint32_t w[V / 2]; ld_words<V / 2>(p, w);
#pragma unroll
        for (int i = 0; i < V / 2; ++i) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
}
template <typename T, int V = Vec<T>::N> __device__ __forceinline__ void vstore(T* p, const float* f) {
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) *(float4*)(p + 4 * i) = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    } else {
        uint32_t w[V / 2];
#pragma unroll
        for (int i = 0; i < V / 2; ++i) w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
        st_words<V / 2>(p, w);
    }
}

template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// Split-bf16 ("bf16x3") planes: the fp32 elementwise passes that feed a convolution write its operand directly as (hi, lo) bf16
// planes (conv_x3.hip): same bytes as the fp32 tensor they replace, and no separate split pass.
template <int V> __device__ __forceinline__ void store_split(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, long e, const float* f) {
    uint32_t h[V / 2], l[V / 2];
#pragma unroll
    for (int k = 0; k < V / 2; ++k) {
        h[k] = pack_bf16x2(f[2 * k], f[2 * k + 1]);
        l[k] = pack_bf16x2(f[2 * k] - __uint_as_float(h[k] << 16), f[2 * k + 1] - __uint_as_float(h[k] & 0xffff0000u));
    }
    st_words<V / 2>(hi + e, h);
    st_words<V / 2>(lo + e, l);
}
// f = hi + lo: the fp32 value of V elements of a split tensor
template <int V> __device__ __forceinline__ void load_planes(const bf16_t* __restrict__ hi, const bf16_t* __restrict__ lo, long e, float* f) {
    float l[V]; vload<bf16_t, V>(hi + e, f); vload<bf16_t, V>(lo + e, l);
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] += l[k];
}

// Max-pool winners: one byte per output element, the tap (dh * 3 + dw) that won
template <int V> __device__ __forceinline__ void unpack_winners(const uint8_t* p, uint32_t* am) {
    uint32_t w[V / 4]; ld_words<V / 4>(p, w);
#pragma unroll
    for (int k = 0; k < V; ++k) am[k] = (w[k / 4] >> (8 * (k & 3))) & 0xff;
}
template <int V> __device__ __forceinline__ void pack_winners(uint8_t* p, const uint32_t* am) {
    uint32_t w[V / 4];
#pragma unroll
    for (int k = 0; k < V / 4; ++k) w[k] = am[4 * k] | (am[4 * k + 1] << 8) | (am[4 * k + 2] << 16) | (am[4 * k + 3] << 24);
    st_words<V / 4>(p, w);
}

// (scale, shift) of V channels from c: the first two rows of a bnp [4][C]
template <int V> __device__ __forceinline__ void load_scale_shift(const float* bnp, int C, int c, float* sc, float* sh) {
#pragma unroll
    for (int k = 0; k < V; ++k) { sc[k] = bnp[c + k]; sh[k] = bnp[C + c + k]; }
}

// Grid-stride loop over the nvec V-element vectors of an [M][C] tensor, 256 threads per workgroup: loadp(c) fetches the parameters
// of channels c .. c + V - 1, body(e) handles the vector at element e.  The grid stride (gridDim * 256 vectors) is a multiple of
// C / V whenever 256 * V % C == 0: the thread's channels are then fixed and loadp runs once.
template <int V, typename LoadP, typename Body>
__device__ __forceinline__ void for_each_vec(long nvec, int C, LoadP loadp, Body body) {
    const bool fixed = ((256 * V) % C) == 0;
    if (fixed) loadp((int)(((long)threadIdx.x * V) % C));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const long e = i * V;
        if (!fixed) loadp((int)(e % C));
        body(e);
    }
}

// rows of the [M][C] matrix reduced by one workgroup: ~1024 workgroups for large M, never fewer than 16 rows (the per-lane
// row loop is a chain of dependent-latency loads; at small M short chains in more workgroups win)
static inline int red_rows(long M) { long r = (M + 1023) / 1024; if (r < 16) r = 16; return (int)((r + 15) / 16 * 16); }

// ---------------------------------------------------------------- row-lane reduction: one partial row (s, q) per workgroup
// A workgroup of 256 threads reduces rows [blockIdx.x * rows_per_block, ...) of an [M][C] matrix over the CS channels from cl0 (a
// channel slice; CS = C, cl0 = 0 for the whole row): CS / V vector lanes along the channels x rl row lanes.  rowop(r, c, s, q) adds
// what row r contributes at channels c .. c + V - 1 to the lane's sums; each lane takes its rows in order, then the row lanes
// are combined through LDS ([rl][CS][2] floats of dynamic shared memory) in lane order: part[blockIdx.x][cl0 .. cl0 + CS][2].
template <int V> __device__ __forceinline__ int row_lane_channel(int CS) { return (int)(threadIdx.x % (CS / V)) * V; }   // within the slice
template <int V, typename RowOp>
__device__ __forceinline__ void row_reduce(long M, int C, int CS, int cl0, int rows_per_block, float* __restrict__ part, RowOp rowop) {
    const int vcs = CS / V;                // vector lanes along channels
    const int rl = 256 / vcs;              // row lanes
    const int cl = row_lane_channel<V>(CS), rr = threadIdx.x / vcs;
    long r0 = (long)blockIdx.x * rows_per_block;
    long r1 = r0 + rows_per_block; if (r1 > M) r1 = M;
    float s[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { s[i] = 0.f; q[i] = 0.f; }
    if (rr < rl)
        for (long r = r0 + rr; r < r1; r += rl) rowop(r, cl0 + cl, s, q);
    extern __shared__ float sm[];
    if (rr < rl)
#pragma unroll
        for (int i = 0; i < V; ++i) { sm[(rr * CS + cl + i) * 2] = s[i]; sm[(rr * CS + cl + i) * 2 + 1] = q[i]; }
    __syncthreads();
    for (int c = threadIdx.x; c < CS; c += 256) {
        float a = 0.f, b = 0.f;
        for (int k = 0; k < rl; ++k) { a += sm[(k * CS + c) * 2]; b += sm[(k * CS + c) * 2 + 1]; }
        part[((long)blockIdx.x * C + cl0 + c) * 2] = a; part[((long)blockIdx.x * C + cl0 + c) * 2 + 1] = b;
    }
}

// column partial sums: (sum x, sum x^2) per block
template <typename T>
__global__ __launch_bounds__(256) void col_stats_kernel(const T* __restrict__ x, long M, int C, int rows_per_block, float* __restrict__ part) {
    constexpr int V = Vec<T>::N;
    row_reduce<V>(M, C, C, 0, rows_per_block, part, [&](long r, int c, float* s, float* q) {
        float f[V]; vload<T>(x + r * C + c, f);
#pragma unroll
        for (int i = 0; i < V; ++i) { s[i] += f[i]; q[i] += f[i] * f[i]; }
    });
}

// Fixed-order reduction of per-workgroup partials part[nparts][C][2] for CPW channels per workgroup of 1024 threads
// (CPW channel lanes x 1024/CPW partial lanes; eight independent loads per lane in flight, double accumulators).  Fewer
// channels per workgroup = more workgroups and fewer dependent load rounds per lane: these launches sit on the step's
// dependency chain, their latency -- not their bandwidth -- is what counts.  Returns the totals in (s, q) for pl == 0.
template <int CPW>
__device__ __forceinline__ void reduce_parts_1024(const float* __restrict__ part, int nparts, int C, int c, double& s, double& q,
                                                  double* sm /* [16][CPW][2] */) {
    constexpr int NPL = 1024 / CPW;
    const int cl = threadIdx.x % CPW, pl = threadIdx.x / CPW;
    double sa[4] = {0, 0, 0, 0}, qa[4] = {0, 0, 0, 0};
    if (c < C) {
        int k = pl;
        for (; k + 7 * NPL < nparts; k += 8 * NPL) {
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *(const float2*)(part + ((long)(k + u * NPL) * C + c) * 2);
#pragma unroll
            for (int u = 0; u < 8; ++u) { sa[u & 3] += v[u].x; qa[u & 3] += v[u].y; }
        }
        for (; k + NPL < nparts; k += 2 * NPL) {
            float2 a = *(const float2*)(part + ((long)k * C + c) * 2), b = *(const float2*)(part + ((long)(k + NPL) * C + c) * 2);
            sa[0] += a.x; qa[0] += a.y; sa[1] += b.x; qa[1] += b.y;
        }
        for (; k < nparts; k += NPL) { float2 a = *(const float2*)(part + ((long)k * C + c) * 2); sa[0] += a.x; qa[0] += a.y; }
    }
    // part-lanes of a wave by butterfly (lane = pl * CPW + cl: xor offsets CPW .. 32), the 16 waves through LDS in wave order
    double a = (sa[0] + sa[1]) + (sa[2] + sa[3]), b = (qa[0] + qa[1]) + (qa[2] + qa[3]);
#pragma unroll
    for (int o = 32; o >= CPW; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < CPW) { sm[(wave * CPW + cl) * 2] = a; sm[(wave * CPW + cl) * 2 + 1] = b; }
    __syncthreads();
    s = 0; q = 0;
    if (pl == 0) for (int k = 0; k < 16; ++k) { s += sm[(k * CPW + cl) * 2]; q += sm[(k * CPW + cl) * 2 + 1]; }
}
static inline int finalize_cpw() {
    // channels per workgroup of the finalize launches: 2, 4 and 8 measure the same end to end (6.25-6.28 ms/step; the
    // launches sit at their ~5 us launch + cross-XCD read latency floor whatever their shape) -- 8 unless AB_BNFIN_CPW says so
    static const int force = getenv("AB_BNFIN_CPW") ? atoi(getenv("AB_BNFIN_CPW")) : 0;
    return (force == 2 || force == 4) ? force : 8;
}

// ---------------------------------------------------------------- BN finalize: partials -> scale/shift, saved stats
// bnp: float [4][C] = scale (gamma*invstd), shift, mean, invstd.  running stats updated in place when non-null.
struct BnChannel { float sc, sh, mean, invstd; double var, n; };   // n: the element count
// one channel's parameters from its sums (s, q) = (sum x, sum x^2) over `count` elements
__device__ __forceinline__ BnChannel bn_params_from_sums(double s, double q, long count, float g, float bt, float eps) {
    BnChannel p;
    p.n = (double)count;
    double mean = s / p.n;
    double var = q / p.n - mean * mean; if (var < 0) var = 0;
    p.invstd = (float)(1.0 / sqrt(var + (double)eps));
    p.sc = g * p.invstd; p.sh = bt - (float)mean * p.sc; p.mean = (float)mean; p.var = var;
    return p;
}
// ... written to column c of bnp
__device__ __forceinline__ void bn_store_params(const BnChannel& p, float* __restrict__ bnp, int C, int c) {
    bnp[c] = p.sc; bnp[C + c] = p.sh; bnp[2 * C + c] = p.mean; bnp[3 * C + c] = p.invstd;
}
// ... folded into the running statistics, whose old values are (rm, rv); the variance as its unbiased estimate
__device__ __forceinline__ void bn_update_running(const BnChannel& p, long count, float momentum, float rm, float rv, float* __restrict__ running_mean,
                                                  float* __restrict__ running_var, int c) {
    double unb = count > 1 ? p.var * p.n / (double)(count - 1) : p.var;
    running_mean[c] = (1.f - momentum) * rm + momentum * p.mean;
    running_var[c] = (1.f - momentum) * rv + momentum * (float)unb;
}
// eval mode: column c of bnp from the running statistics
__device__ __forceinline__ void bn_eval_params_one(int C, int c, const float* gamma, const float* beta, const float* rm, const float* rv,
                                                   float eps, float* bnp) {
    float invstd = 1.f / sqrtf(rv[c] + eps);
    float sc = gamma[c] * invstd;
    bnp[c] = sc; bnp[C + c] = beta[c] - rm[c] * sc; bnp[2 * C + c] = rm[c]; bnp[3 * C + c] = invstd;
}
// the backward's sums of channel c: dbeta = sum dz, dgamma = sum dz * xhat, and both again as bwdp [2][C]
__device__ __forceinline__ void bn_store_bwd_sums(double s, double q, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                  float* __restrict__ bwdp, int C, int c) {
    dbeta[c] = (float)s; dgamma[c] = (float)q;
    bwdp[c] = (float)s; bwdp[C + c] = (float)q;
}

// block = CPW channels x 1024/CPW part-lanes, grid = ceil(C/CPW)
template <int CPW>
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ part, int nparts, int C, long count,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, float momentum, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var, float* __restrict__ bnp) {
    const int cl = threadIdx.x % CPW, pl = threadIdx.x / CPW;
    const int c = blockIdx.x * CPW + cl;
    __shared__ double sm[16 * CPW * 2];
    // the finishing thread's parameters are requested before the reduction so their latency hides under it
    float g = 0.f, bt = 0.f, rm = 0.f, rv = 0.f;
    const bool fin = pl == 0 && c < C;
    if (fin) { g = gamma[c]; bt = beta[c]; if (running_mean) { rm = running_mean[c]; rv = running_var[c]; } }
    double s, q; reduce_parts_1024<CPW>(part, nparts, C, c, s, q, sm);
    if (fin) {
        const BnChannel p = bn_params_from_sums(s, q, count, g, bt, eps);
        bn_store_params(p, bnp, C, c);
        if (running_mean) bn_update_running(p, count, momentum, rm, rv, running_mean, running_var, c);
    }
}

// eval-mode: scale/shift from running statistics
__global__ void bn_eval_params_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, float* bnp) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_eval_params_one(C, c, gamma, beta, rm, rv, eps, bnp);
}

// every BatchNorm of a network in ONE launch: desc[n][6] = (gamma offset, beta offset in `flat`; running_mean, running_var offset in
// `stats`; output offset in `out`; C) -- see ab_bn_eval_params_batch
__global__ void bn_eval_params_batch_kernel(const float* __restrict__ flat, const float* __restrict__ stats, const int* __restrict__ desc,
                                            float eps, float* __restrict__ out) {
    const int* d = desc + blockIdx.y * 6;
    const int C = d[5];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_eval_params_one(C, c, flat + d[0], flat + d[1], stats + d[2], stats + d[3], eps, out + d[4]);
}

// ---------------------------------------------------------------- BN apply (+residual) (+ReLU)
// Forward elementwise body: f = [relu]( f*sc + sh [+ r] ) in fp32, the expression the folded conv epilogues and every backward mask
// repeat.  RES says where the residual r comes from:
enum {
    RES_F32 = 0,       // none (res == NULL) or an fp32 tensor `res`
    RES_PLANES = 1,    // its (hi, lo) planes res_hi, res_lo; `res` unused -- the block input need not exist in fp32
    RES_RAWBN = 2,     // `res` is itself a raw conv output and the residual is res*sc2 + sh2 (the downsample branch, resnet.py:95-99:
                       // its BatchNorm output is never materialised)
    RES_ANY = 3        // RES_F32 or RES_PLANES, told apart by res_hi != NULL at run time (the 4-channel form)
};
// loads r; false: there is no residual
template <int V, int RES>
__device__ __forceinline__ bool load_res(const float* __restrict__ res, const bf16_t* __restrict__ res_hi, const bf16_t* __restrict__ res_lo,
                                         long e, float* r) {
    if (RES == RES_PLANES || (RES == RES_ANY && res_hi)) { load_planes<V>(res_hi, res_lo, e, r); return true; }
    if (res) vload<float, V>(res + e, r);
    return res != nullptr;
}
template <int V, int RES>
__device__ __forceinline__ void bn_fwd_elem(float* f, float* r, bool has_res, const float* sc, const float* sh, const float* sc2, const float* sh2, int relu) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float v = f[k] * sc[k] + sh[k];
        if constexpr (RES == RES_RAWBN) r[k] = r[k] * sc2[k] + sh2[k];
        if (has_res) v += r[k];
        if (relu) v = fmaxf(v, 0.f);
        f[k] = v;
    }
}
// ... of the V fp32 elements at e, stored as fp32 `out` (optional) and as split planes
template <int V, int RES>
__device__ __forceinline__ void bn_fwd_x3(long e, const float* __restrict__ y, const float* __restrict__ res, const bf16_t* __restrict__ res_hi,
                                          const bf16_t* __restrict__ res_lo, const float* sc, const float* sh, const float* sc2, const float* sh2,
                                          int relu, float* __restrict__ out, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    float f[V], r[V];
    vload<float, V>(y + e, f);
    const bool has_res = load_res<V, RES>(res, res_hi, res_lo, e, r);
    bn_fwd_elem<V, RES>(f, r, has_res, sc, sh, sc2, sh2, relu);
    if (out) vstore<float, V>(out + e, f);
    store_split<V>(hi, lo, e, f);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const T* __restrict__ res,
                                                       const float* __restrict__ bnp, long nvec, int C, int relu,
                                                       T* __restrict__ out) {
    constexpr int V = Vec<T>::N;
    float sc[V], sh[V];
    for_each_vec<V>(nvec, C, [&](int c) { load_scale_shift<V>(bnp, C, c, sc, sh); }, [&](long e) {
        float f[V]; vload<T>(y + e, f);
        float r[V];
        if (res) vload<T>(res + e, r);
        bn_fwd_elem<V, RES_F32>(f, r, res != nullptr, sc, sh, nullptr, nullptr, relu);
        vstore<T>(out + e, f);
    });
}

// ---------------------------------------------------------------- 3x3/2 max-pool gradient gathers (see the pooling kernels below)
// gradient of the 3x3/2 max-pool input at row r = (n,h,w) of the [N*H*W][C] map, channels c .. c + V - 1: sum over the <= 4 windows
// that cover the pixel of dpool where the recorded winner is this pixel (what maxpool_bwd_kernel stores, rounded to T the same way)
template <typename T>
__device__ __forceinline__ void pool_gather(const uint8_t* __restrict__ idx, const T* __restrict__ dpool, long r, int H, int W, int C, int c, float* acc) {
    constexpr int V = Vec<T>::N;
    const int Ho = H / 2, Wo = W / 2;
    const int w = (int)(r % W); const long t = r / W; const int h = (int)(t % H), n = (int)(t / H);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int ho = h / 2; ho <= (h + 1) / 2; ++ho) {
        if (ho >= Ho) continue;
        int dh = h - (ho * 2 - 1);
        for (int wo = w / 2; wo <= (w + 1) / 2; ++wo) {
            if (wo >= Wo) continue;
            int code = dh * 3 + (w - (wo * 2 - 1));
            long o = (((long)n * Ho + ho) * Wo + wo) * C + c;
            uint32_t am[V]; unpack_winners<V>(idx + o, am);
            float g[V]; vload<T>(dpool + o, g);
#pragma unroll
            for (int k = 0; k < V; ++k) if (am[k] == code) acc[k] += g[k];
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = round_to<T>(acc[k]);
}
// ... of the input row PAIR (2p, 2p+1) at column w, channels c .. c + V - 1 (acc0, acc1; not rounded): row 2p lies in pooled row p
// only, row 2p+1 in p and p+1 -- the winners / gradients of pooled row p are loaded once for both (4 loads of each kind instead of 6)
template <typename T, int V>
__device__ __forceinline__ void pool_gather_pair(const uint8_t* __restrict__ idx, const T* __restrict__ dout, int n, int p, int w, int Ho, int Wo,
                                                 int C, int c, float* acc0, float* acc1) {
#pragma unroll
    for (int k = 0; k < V; ++k) { acc0[k] = 0.f; acc1[k] = 0.f; }
#pragma unroll
    for (int dp = 0; dp < 2; ++dp) {
        const int ho = p + dp;
        if (ho >= Ho) continue;
        for (int wo = w / 2; wo <= (w + 1) / 2; ++wo) {
            if (wo >= Wo) continue;
            const int cw = w - (wo * 2 - 1);
            const long o = (((long)n * Ho + ho) * Wo + wo) * C + c;
            uint32_t am[V]; unpack_winners<V>(idx + o, am);
            float g[V]; vload<T, V>(dout + o, g);
            // window rows of pooled row ho: 2ho-1 .. 2ho+1.  dp = 0: input row 2p is its row 1, row 2p+1 its row 2;
            // dp = 1: input row 2p+1 is row 0 of pooled row p+1.  (Selects, not `if (...) acc += g`: the conditional statement
            // compiled to EXEC-masked branches with an element of g loaded under one of them, +1 % on pool_bwd_bn_apply_x3.)
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int a = (int)am[k];
                if (dp == 0) {
                    acc0[k] = (a == 3 + cw) ? acc0[k] + g[k] : acc0[k];
                    acc1[k] = (a == 6 + cw) ? acc1[k] + g[k] : acc1[k];
                } else {
                    acc1[k] = (a == cw) ? acc1[k] + g[k] : acc1[k];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- BN backward
// Backward elementwise bodies, for V channels whose parameters sit in a BnBwd:
//   relu_mask    dz = dout where the ReLU passed, else 0
//   bn_bwd_sums  s += dz, q += dz * xhat                                  (pass 1)
//   bn_bwd_dy    dy = gamma*invstd * (dz - mean(dz) - xhat * mean(dz*xhat))  (pass 2)
enum { RELU_NONE = 0, RELU_OUT = 1, RELU_RECOMPUTE = 2 };      // the `relu` argument of the backward entry points
template <int V> struct BnBwd { float ga[V], sh[V], mu[V], is[V], k1[V], k2[V]; };   // gamma*invstd, shift, mean, invstd, mean(dz), mean(dz*xhat)
template <int V> __device__ __forceinline__ void load_bn_stats(BnBwd<V>& P, const float* __restrict__ bnp, int C, int c) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        P.ga[k] = bnp[c + k]; P.sh[k] = bnp[C + c + k];
        P.mu[k] = bnp[2 * C + c + k]; P.is[k] = bnp[3 * C + c + k];
    }
}
// ... and the means from the channel sums: sums [2][S] = (sum dz, sum dz * xhat), read from channel cs (bwdp with S = C and
// cs = c, or the 64 channels of a workgroup's own finalize)
template <int V>
__device__ __forceinline__ void load_bwd_params(BnBwd<V>& P, const float* __restrict__ bnp, int C, int c, const float* sums, int S, int cs, float invM) {
    load_bn_stats<V>(P, bnp, C, c);
#pragma unroll
    for (int k = 0; k < V; ++k) { P.k1[k] = sums[cs + k] * invM; P.k2[k] = sums[S + cs + k] * invM; }
}
// the stored activation for the relu == 1 mask: `out`, or the hi plane of the split activation (fp32 tensors only: same sign,
// half the bytes of the fp32 copy)
template <typename T, int V>
__device__ __forceinline__ void load_relu_out(int relu, const T* __restrict__ out, const bf16_t* __restrict__ out_hi, long e, float* o) {
    if (relu != RELU_OUT) return;
    if (out_hi) vload<bf16_t, V>(out_hi + e, o); else vload<T, V>(out + e, o);
}
// g: dout -> dz.  relu == 1: the mask from the stored activation o; relu == 2: recomputed from y with bn_apply's own expression (same
// f32 value that was clamped and stored), which saves reading the activation (o is not read); relu == 0: none
template <int V> __device__ __forceinline__ void relu_mask(const BnBwd<V>& P, int relu, float* g, const float* o, const float* yy) {
    if (relu == RELU_OUT) {
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = (o[k] > 0.f) ? g[k] : 0.f;
    } else if (relu == RELU_RECOMPUTE) {
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = (yy[k] * P.ga[k] + P.sh[k] > 0.f) ? g[k] : 0.f;
    }
}
template <int V> __device__ __forceinline__ void bn_bwd_sums(const BnBwd<V>& P, const float* dz, const float* yy, float* s, float* q) {
#pragma unroll
    for (int k = 0; k < V; ++k) { s[k] += dz[k]; q[k] += dz[k] * ((yy[k] - P.mu[k]) * P.is[k]); }
}
template <int V> __device__ __forceinline__ void bn_bwd_dy(const BnBwd<V>& P, const float* dz, const float* yy, float* d) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float xhat = (yy[k] - P.mu[k]) * P.is[k];
        d[k] = P.ga[k] * (dz[k] - P.k1[k] - xhat * P.k2[k]);
    }
}
// pass 2 on the 8 fp32 elements at e, dy written as split planes (its only consumers are the data- and weight-gradient convs),
// dz optionally as fp32 (the residual gradient)
__device__ __forceinline__ void bn_bwd_x3(const BnBwd<8>& P, long e, const float* __restrict__ dout, const float* __restrict__ out,
                                          const bf16_t* __restrict__ out_hi, const float* __restrict__ y, int relu, bf16_t* __restrict__ dy_hi,
                                          bf16_t* __restrict__ dy_lo, float* __restrict__ dz_out) {
    float g[8], o[8], yy[8], d[8];
    vload<float, 8>(dout + e, g);
    vload<float, 8>(y + e, yy);
    load_relu_out<float, 8>(relu, out, out_hi, e, o);
    relu_mask<8>(P, relu, g, o, yy);
    bn_bwd_dy<8>(P, g, yy, d);
    store_split<8>(dy_hi, dy_lo, e, d);
    if (dz_out) vstore<float, 8>(dz_out + e, g);
}

// pass 1: dz = dout * (out > 0 if relu); partial sums of dz and dz * xhat per channel
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                            const T* __restrict__ y, const float* __restrict__ bnp,
                                                            long M, int C, int relu, int rows_per_block, float* __restrict__ part,
                                                            const uint8_t* __restrict__ pool_idx = nullptr, int pH = 0, int pW = 0,
                                                            const bf16_t* __restrict__ out_hi = nullptr) {
    constexpr int V = Vec<T>::N;
    // wide tensors (C / V > 256: the 2048-channel stage of the Bottleneck ResNets): gridDim.y slices of CS = C / gridDim.y channels
    const int CS = C / (int)gridDim.y, cl0 = (int)blockIdx.y * CS;
    BnBwd<V> P; load_bn_stats<V>(P, bnp, C, cl0 + row_lane_channel<V>(CS));
    row_reduce<V>(M, C, CS, cl0, rows_per_block, part, [&](long r, int c, float* s, float* q) {
        const long e = r * C + c;
        float g[V], o[V], yy[V];
        if (pool_idx) pool_gather<T>(pool_idx, dout, r, pH, pW, C, c, g);   // dout is the POOLED gradient: gather this pixel's share (fused max-pool backward)
        else vload<T>(dout + e, g);
        vload<T>(y + e, yy);
        load_relu_out<T, V>(relu, out, out_hi, e, o);
        relu_mask<V>(P, relu, g, o, yy);
        bn_bwd_sums<V>(P, g, yy, s, q);
    });
}

// reduce partials -> dgamma, dbeta (written to the flat grad buffer) and bwdp[2][C] = (sum dz, sum dz*xhat)
template <int CPW>
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ part, int nparts, int C,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ bwdp) {
    const int cl = threadIdx.x % CPW, pl = threadIdx.x / CPW;
    const int c = blockIdx.x * CPW + cl;
    __shared__ double sm[16 * CPW * 2];
    double s, q; reduce_parts_1024<CPW>(part, nparts, C, c, s, q, sm);
    if (pl == 0 && c < C) bn_store_bwd_sums(s, q, dgamma, dbeta, bwdp, C, c);
}

// pass 2: dy;  optionally also writes dz (residual gradient)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                           const T* __restrict__ y, const float* __restrict__ bnp,
                                                           const float* __restrict__ bwdp, long nvec, int C, long M,
                                                           int relu, T* __restrict__ dy, T* __restrict__ dz_out,
                                                           const uint8_t* __restrict__ pool_idx = nullptr, int pH = 0, int pW = 0) {
    constexpr int V = Vec<T>::N;
    const float invM = 1.f / (float)M;
    BnBwd<V> P;
    for_each_vec<V>(nvec, C, [&](int c) { load_bwd_params<V>(P, bnp, C, c, bwdp, C, c, invM); }, [&](long e) {
        float g[V], o[V], yy[V], d[V];
        if (pool_idx) { const long r = e / C; pool_gather<T>(pool_idx, dout, r, pH, pW, C, (int)(e - r * C), g); }
        else vload<T>(dout + e, g);
        vload<T>(y + e, yy);
        load_relu_out<T, V>(relu, out, nullptr, e, o);
        relu_mask<V>(P, relu, g, o, yy);
        bn_bwd_dy<V>(P, g, yy, d);
        vstore<T>(dy + e, d);
        if (dz_out) vstore<T>(dz_out + e, g);
    });
}

// ---------------------------------------------------------------- elementwise add (gradient accumulation)
template <typename T>
__global__ __launch_bounds__(256) void add_kernel(const T* __restrict__ a, const T* __restrict__ b, long nvec, T* __restrict__ out) {
    constexpr int V = Vec<T>::N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        float x[V], y[V]; vload<T>(a + i * V, x); vload<T>(b + i * V, y);
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] += y[k];
        vstore<T>(out + i * V, x);
    }
}

// ---------------------------------------------------------------- 3x3 / stride 2 / pad 1 max-pool (resnet.py:157)
// forward also records WHICH of the 9 taps won (first maximum in row-major scan order == torch semantics), one byte
// per output element; backward then gathers from the <= 4 windows covering an input pixel without re-reading x.
// bnp != nullptr: the input is a raw conv output and relu(x*scale+shift), rounded to T exactly as ab_bn_apply would store
// it, is pooled instead (the activation tensor is never materialised).
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ bnp, int N, int H,
                                                          int W, int C, T* __restrict__ out, uint8_t* __restrict__ idx,
                                                          bf16_t* __restrict__ out_hi = nullptr, bf16_t* __restrict__ out_lo = nullptr) {
    constexpr int V = Vec<T>::N;
    const int Ho = H / 2, Wo = W / 2, vc = C / V;
    // grid (ceil(Wo*vc / 256), Ho, N): one output row per (blockIdx.y, blockIdx.z) -- no 64-bit div/mod per vector (they dominated the
    // flat-index version of this HBM-bound kernel)
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    if (col < (unsigned)(Wo * vc)) {
        const int wo = (int)(col / (unsigned)vc), cv = (int)(col - (unsigned)wo * vc);
        const int n = blockIdx.z, ho = blockIdx.y;
        const long i = (((long)n * Ho + ho) * Wo + wo) * vc + cv;
        float m[V]; uint32_t am[V];
        float sc[V], sh[V];
        if (bnp) load_scale_shift<V>(bnp, C, cv * V, sc, sh);
#pragma unroll
        for (int k = 0; k < V; ++k) { m[k] = -INFINITY; am[k] = 0; }
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            int h = ho * 2 + dh - 1; if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                int w = wo * 2 + dw - 1; if ((unsigned)w >= (unsigned)W) continue;
                float f[V]; vload<T>(x + (((long)n * H + h) * W + w) * C + cv * V, f);
                if (bnp) {
#pragma unroll
                    for (int k = 0; k < V; ++k) f[k] = round_to<T>(fmaxf(f[k] * sc[k] + sh[k], 0.f));
                }
#pragma unroll
                for (int k = 0; k < V; ++k) if (f[k] > m[k]) { m[k] = f[k]; am[k] = dh * 3 + dw; }
            }
        }
        vstore<T>(out + i * V, m);
        if constexpr (V == 4) {
            // fp32 path: the pooled tensor also as (hi, lo) planes for the split-bf16 convolutions that read it
            if (out_hi) store_split<4>(out_hi, out_lo, i * 4, m);
        }
        if (idx) pack_winners<V>(idx + i * V, am);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint8_t* __restrict__ idx, const T* __restrict__ dout,
                                                          int N, int H, int W, int C, T* __restrict__ dx) {
    constexpr int V = Vec<T>::N;
    const int Ho = H / 2, Wo = W / 2, vc = C / V;
    // grid (ceil(W*vc / 256), H/2, N): a thread owns one channel vector of the input row PAIR (2p, 2p+1) -- half the workgroups of
    // one row per thread; 32-bit index math only
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    if (col < (unsigned)(W * vc)) {
        const int w = (int)(col / (unsigned)vc), cv = (int)(col - (unsigned)w * vc);
        const int n = blockIdx.z, p = blockIdx.y;
        float acc0[V], acc1[V];
        pool_gather_pair<T, V>(idx, dout, n, p, w, Ho, Wo, C, cv * V, acc0, acc1);
        const long i = (((long)n * H + 2 * p) * W + w) * vc + cv;
        vstore<T>(dx + i * V, acc0);
        vstore<T>(dx + (i + (long)W * vc) * V, acc1);
    }
}

// Backward of maxpool3x3/2(relu(bn(y))) for the fp32 path, first half: the row-pair max-pool backward above with the BatchNorm
// backward's mask + reduction riding on it.  A thread owns one channel vector of RP input row pairs; per row it gathers the
// pooled gradient, recomputes the ReLU mask from y (bn_apply's own expression), stores the MASKED gradient dz and keeps
// sum(dz), sum(dz * xhat) for its four channels; the 16 threads of a workgroup that share a channel vector combine through LDS:
// one partial row per workgroup.  Replaces the separate reduction pass over (da, y) -- 0.54 GB at the benchmark size.
template <int RP, bool WRITE_DZ = true>
__global__ __launch_bounds__(256) void pool_bwd_bn_reduce_kernel(const uint8_t* __restrict__ idx, const float* __restrict__ dout,
                                                                  const float* __restrict__ y, const float* __restrict__ bnp,
                                                                  int N, int H, int W, int C, float* __restrict__ dz,
                                                                  float* __restrict__ part) {
    const int Ho = H / 2, Wo = W / 2, vc = C / 4;
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    const bool ok = col < (unsigned)(W * vc);
    const int w = ok ? (int)(col / (unsigned)vc) : 0, cv = ok ? (int)(col - (unsigned)w * vc) : 0;
    const int n = blockIdx.z;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    BnBwd<4> P; load_bn_stats<4>(P, bnp, C, cv * 4);
    if (ok)
        for (int rp = 0; rp < RP; ++rp) {
            const int p = blockIdx.y * RP + rp;
            if (p >= Ho) break;
            float acc0[4], acc1[4], ya[4], yb[4];
            pool_gather_pair<float, 4>(idx, dout, n, p, w, Ho, Wo, C, cv * 4, acc0, acc1);
            const long i = ((((long)n * H + 2 * p) * W + w) * vc + cv) * 4;
            vload<float, 4>(y + i, ya);
            vload<float, 4>(y + i + (long)W * C, yb);
            relu_mask<4>(P, RELU_RECOMPUTE, acc0, nullptr, ya);
            relu_mask<4>(P, RELU_RECOMPUTE, acc1, nullptr, yb);
            bn_bwd_sums<4>(P, acc0, ya, s, q);
            bn_bwd_sums<4>(P, acc1, yb, s, q);
            if constexpr (WRITE_DZ) {
                vstore<float, 4>(dz + i, acc0);
                vstore<float, 4>(dz + i + (long)W * C, acc1);
            }
        }
    // threads sharing cv: tid % vc (vc divides 256 for C = 64 .. 1024); fixed-order combine
    extern __shared__ float sm[];                          // [256][8]
#pragma unroll
    for (int k = 0; k < 4; ++k) { sm[threadIdx.x * 8 + k] = ok ? s[k] : 0.f; sm[threadIdx.x * 8 + 4 + k] = ok ? q[k] : 0.f; }
    __syncthreads();
    const long prow = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        const int cvv = c >> 2, k = c & 3;
        float a = 0.f, b = 0.f;
        // this workgroup's threads with channel vector cvv: t = cvv - first_cv (mod vc) + j * vc
        const unsigned col0 = blockIdx.x * 256;
        int t0 = (int)((cvv + vc - (int)(col0 % (unsigned)vc)) % vc);
        for (int t = t0; t < 256; t += vc) { a += sm[t * 8 + k]; b += sm[t * 8 + 4 + k]; }
        part[(prow * C + c) * 2] = a; part[(prow * C + c) * 2 + 1] = b;
    }
}

// ---------------------------------------------------------------- global average pool (resnet.py:219) fwd / bwd
// grid (N, ceil(C / (32*V))): 32 channel-vector lanes x 8 pixel lanes per workgroup, pixel-lane partials combined in
// fixed order through LDS
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ x, int HW, int C, float* __restrict__ out) {
    constexpr int V = Vec<T>::N;
    __shared__ float sm[8][32 * V + 1];
    const int n = blockIdx.x, cv = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cv) * V;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    if (c0 < C)
        for (int p = pl; p < HW; p += 8) {
            float f[V]; vload<T>(x + ((long)n * HW + p) * C + c0, f);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += f[k];
        }
#pragma unroll
    for (int k = 0; k < V; ++k) sm[pl][cv * V + k] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < 32 * V; c += 256) {
        int cg = blockIdx.y * 32 * V + c;
        if (cg >= C) continue;
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += sm[k][c];
        out[(long)n * C + cg] = t / (float)HW;
    }
}
// dx[n,p,c] (+)= g[n,c] / HW  (one 16-byte vector per thread)
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ g, int HW, int C, long nvec,
                                                          T* __restrict__ dx, int accumulate) {
    constexpr int V = Vec<T>::N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        long e = i * V;
        int c = (int)(e % C); long n = e / ((long)HW * C);
        float v[V];
        if (accumulate) vload<T>(dx + e, v);
#pragma unroll
        for (int k = 0; k < V; ++k) { float t = g[n * C + c + k] / (float)HW; v[k] = accumulate ? v[k] + t : t; }
        vstore<T>(dx + e, v);
    }
}

// ---------------------------------------------------------------- precision / layout packing
__global__ void cast_f32_bf16_kernel(const float* __restrict__ src, long n, bf16_t* __restrict__ dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = f32_to_bf16(src[i]);
}
// src [O][K][I] (OHWI, K = kh*kw) -> dst [I][K][O], optionally converting to bf16
template <typename T>
__global__ void transpose_oki_kernel(const float* __restrict__ src, int O, int K, int I, T* __restrict__ dst) {
    long n = (long)O * K * I;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        int o = (int)(e % O); long t = e / O; int k = (int)(t % K); int i = (int)(t / K);
        st_f32(dst + e, src[((long)o * K + k) * I + i]);
    }
}
// All dgrad weight copies in one launch: tensor t = desc[t] (see ab_transpose_desc), a workgroup moves one 64(o) x 64(i)
// tile of one tap k through LDS: 256-byte coalesced row reads of src [O][K][I], 16-byte stores into dst [I][K][O].
// LO_OFF != 0 (T = bf16 only): also write the lo plane bf16(v - hi) at dst + lo_off elements (split-bf16 IHWO copies)
template <typename T>
__global__ __launch_bounds__(256) void transpose_oki_batch_kernel(const ab_transpose_desc* __restrict__ desc, int ntensors, long lo_off = 0) {
    __shared__ float sm[64][65];
    int t = 0;
    while (t + 1 < ntensors && (long)blockIdx.x >= desc[t + 1].tile_begin) ++t;
    const ab_transpose_desc d = desc[t];
    const int O = d.O, K = d.K, I = d.I;
    const int ti = (I + 63) / 64;
    long tile = (long)blockIdx.x - d.tile_begin;
    const int it = (int)(tile % ti); tile /= ti;
    const int k = (int)(tile % K); const int ot = (int)(tile / K);
    const int o0 = ot * 64, i0 = it * 64;
    const float* __restrict__ src = (const float*)d.src;
    T* __restrict__ dst = (T*)d.dst;
    {
        const int c4 = (threadIdx.x & 15) * 4, r = threadIdx.x >> 4;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            int o = o0 + r + pass * 16, i = i0 + c4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (o < O && i < I) v = *(const float4*)(src + ((long)o * K + k) * I + i);
            sm[r + pass * 16][c4] = v.x; sm[r + pass * 16][c4 + 1] = v.y; sm[r + pass * 16][c4 + 2] = v.z; sm[r + pass * 16][c4 + 3] = v.w;
        }
    }
    __syncthreads();
    {
        constexpr int V = Vec<T>::N;                 // 8 bf16 / 4 f32 per 16-byte store
        constexpr int CL = 64 / V, RP = 256 / CL;    // column lanes, rows per pass
        const int cv = (threadIdx.x % CL) * V, r = threadIdx.x / CL;
#pragma unroll
        for (int pass = 0; pass < 64 / RP; ++pass) {
            int il = r + pass * RP;
            int i = i0 + il, o = o0 + cv;
            if (i < I && o < O) {
                float f[V];
#pragma unroll
                for (int q = 0; q < V; ++q) f[q] = sm[cv + q][il];
                vstore<T>(dst + ((long)i * K + k) * O + o, f);
                if (lo_off) {
#pragma unroll
                    for (int q = 0; q < V; ++q) f[q] -= round_to<T>(f[q]);
                    vstore<T>(dst + lo_off + ((long)i * K + k) * O + o, f);
                }
            }
        }
    }
}

// image NCHW float [N,3,H,W] -> zero-bordered NHWC4 [N, H+6, W+8, 4] in T (border 3 px, channel 3 = 0)
template <typename T>
__global__ void image_pad_kernel(const float* __restrict__ img, int N, int H, int W, T* __restrict__ out) {
    const int Hp = H + 6, Wp = W + 8;
    long n = (long)N * Hp * Wp;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        int wp = (int)(e % Wp); long t = e / Wp; int hp = (int)(t % Hp); int b = (int)(t / Hp);
        int h = hp - 3, w = wp - 3;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
            for (int c = 0; c < 3; ++c) v[c] = img[(((long)b * 3 + c) * H + h) * W + w];
        for (int c = 0; c < 4; ++c) st_f32(out + e * 4 + c, v[c]);
    }
}

// ---------------------------------------------------------------- ReLU backward, column-sum finalize (bias grads)
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ out, long nvec, T* __restrict__ dz) {
    constexpr int V = Vec<T>::N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        float g[V], o[V]; vload<T>(dout + i * V, g); vload<T>(out + i * V, o);
#pragma unroll
        for (int k = 0; k < V; ++k) g[k] = (o[k] > 0.f) ? g[k] : 0.f;
        vstore<T>(dz + i * V, g);
    }
}
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ out) {
    const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl;
    double s = 0.0;
    if (c < C) for (int k = pl; k < nparts; k += 32) s += part[((long)k * C + c) * 2];
    __shared__ double sm[32][8];
    sm[pl][cl] = s;
    __syncthreads();
    if (pl == 0 && c < C) { for (int k = 1; k < 32; ++k) s += sm[k][cl]; out[c] = (float)s; }
}

// ================================================================ split-bf16 ("bf16x3") producers: fp32 in, 8 channels per thread
// out = [relu]( y*scale + shift [+ res] ) -> fp32 `out` (optional) and split planes; the residual forms: RES_* above
// (RESBN is a template parameter: as a run-time branch the second parameter set doubled the time of EVERY launch of this kernel,
// 540 -> 1 005 us per step over its 34 launches)
template <bool RESBN, bool RESPL = false>
__global__ __launch_bounds__(256) void bn_apply_x3_kernel(const float* __restrict__ y, const float* __restrict__ res,
                                                          const float* __restrict__ bnp, long nvec, int C, int relu,
                                                          float* __restrict__ out, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                                          const float* __restrict__ res_bnp = nullptr,
                                                          const bf16_t* __restrict__ res_hi = nullptr,
                                                          const bf16_t* __restrict__ res_lo = nullptr) {
    constexpr int RES = RESPL ? RES_PLANES : RESBN ? RES_RAWBN : RES_F32;
    float sc[8], sh[8], sc2[RESBN ? 8 : 1], sh2[RESBN ? 8 : 1];
    for_each_vec<8>(nvec, C, [&](int c) {
        load_scale_shift<8>(bnp, C, c, sc, sh);
        if constexpr (RESBN) load_scale_shift<8>(res_bnp, C, c, sc2, sh2);
    }, [&](long e) { bn_fwd_x3<8, RES>(e, y, res, res_hi, res_lo, sc, sh, sc2, sh2, relu, out, hi, lo); });
}

// ... for C % 8 == 4 (no layer of the models: the route of a convolution whose fold the conv kernels refuse, and the head with a channel
// count that is a multiple of 4 only): 4 channels per thread
__global__ __launch_bounds__(256) void bn_apply_x3_c4_kernel(const float* __restrict__ y, const float* __restrict__ res,
                                                             const float* __restrict__ bnp, long nvec, int C, int relu,
                                                             float* __restrict__ out, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                                             const bf16_t* __restrict__ res_hi, const bf16_t* __restrict__ res_lo) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const long e = i * 4;
        float sc[4], sh[4]; load_scale_shift<4>(bnp, C, (int)(e % C), sc, sh);
        bn_fwd_x3<4, RES_ANY>(e, y, res, res_hi, res_lo, sc, sh, nullptr, nullptr, relu, out, hi, lo);
    }
}

// BatchNorm-backward pass 2 with dy written as split planes
__global__ __launch_bounds__(256) void bn_bwd_apply_x3_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                              const float* __restrict__ y, const float* __restrict__ bnp,
                                                              const float* __restrict__ bwdp, long nvec, int C, long M, int relu,
                                                              bf16_t* __restrict__ dy_hi, bf16_t* __restrict__ dy_lo,
                                                              float* __restrict__ dz_out, const bf16_t* __restrict__ out_hi) {
    const float invM = 1.f / (float)M;
    BnBwd<8> P;
    for_each_vec<8>(nvec, C, [&](int c) { load_bwd_params<8>(P, bnp, C, c, bwdp, C, c, invM); },
                    [&](long e) { bn_bwd_x3(P, e, dout, out, out_hi, y, relu, dy_hi, dy_lo, dz_out); });
}

// ---------------------------------------------------------------- BatchNorm finalize INSIDE the apply passes (round 4)
// The 76 bn_finalize / bn_bwd_finalize launches of a step (~5 us each: a launch + one dependent reduction over the partial rows) sit on the
// step's dependency chain between the convolution that leaves the per-tile sums and the elementwise pass that needs (scale, shift).  Where
// the partial rows are few (<= BNFIN_MAX_ROWS = 64: layers 3 - 4; measured per step at B = 64: off 9.72 ms, rows <= 32 9.69, <= 64 9.66, <= 256 9.73 --
// at 256 rows the prologue's 64 dependent row loads per lane cost more than the launch they replace) the apply pass reduces them itself: a workgroup owns a SLICE of 64
// channels (256 B of every pixel's fp32 row, 128 B of each plane -- whole cache lines) over a strip of pixels, so its prologue reads only
// rows x 64 x 8 bytes (16 - 128 KB from L2) with 4 row-lanes per channel, fixed summation order (rows r = lane, lane + 4, ... in a double
// each, then the four lanes in order): deterministic.  The workgroup of pixel strip 0 writes bnp / the running statistics / dgamma, dbeta
// for its slice.
#define BNFIN_MAX_ROWS 64
#define BNFIN_SLICE 64

// (s, q) = column sums of part[nparts][C][2] for channel c0 + (tid & 63); valid in every thread after the call
__device__ __forceinline__ void bnfin_reduce(const float* __restrict__ part, int nparts, int C, int c0, double* sm /* [4][64][2] */, double& s, double& q) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    double a = 0, b = 0;
#pragma unroll 4
    for (int r = rl; r < nparts; r += 4) { const float2 v = *(const float2*)(part + ((long)r * C + c0 + cl) * 2); a += v.x; b += v.y; }
    sm[(rl * 64 + cl) * 2] = a; sm[(rl * 64 + cl) * 2 + 1] = b;
    __syncthreads();
    s = ((sm[cl * 2] + sm[(64 + cl) * 2]) + sm[(128 + cl) * 2]) + sm[(192 + cl) * 2];
    q = ((sm[cl * 2 + 1] + sm[(64 + cl) * 2 + 1]) + sm[(128 + cl) * 2 + 1]) + sm[(192 + cl) * 2 + 1];
}
// the workgroup's place: channel slice from c0, pixel strip `strip` of `nstrips`; a thread takes channels c0 + j * 8 .. of the pixels
// strip * 32 + pl, + nstrips * 32, ... (8 channel groups of a pixel, 32 pixels per pass)
struct BnFinTile { int c0, strip, nstrips, j, pl; };
__device__ __forceinline__ BnFinTile bnfin_tile(int C) {
    const int nsl = C / BNFIN_SLICE;
    return {(int)(blockIdx.x % nsl) * BNFIN_SLICE, (int)(blockIdx.x / nsl), (int)(gridDim.x / nsl), (int)(threadIdx.x & 7), (int)(threadIdx.x >> 3)};
}

struct BnFinArgs {
    const float* part; int nparts; long count; const float* gamma; const float* beta; float eps, momentum;
    float* running_mean; float* running_var; float* bnp;      // bnp [4][C]: written by the strip-0 workgroups
};

// RES: RES_F32, RES_PLANES or RES_RAWBN
template <int RES>
__global__ __launch_bounds__(256) void bn_fin_apply_x3_kernel(BnFinArgs fa, const float* __restrict__ y, const float* __restrict__ res,
                                                              const bf16_t* __restrict__ res_hi, const bf16_t* __restrict__ res_lo,
                                                              const float* __restrict__ res_bnp, long M, int C, int relu,
                                                              float* __restrict__ out, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    __shared__ double sm[4 * 64 * 2];
    __shared__ float par[2][BNFIN_SLICE];          // (scale, shift) of the slice: a bnp of 64 channels
    const BnFinTile t = bnfin_tile(C);
    double s, q; bnfin_reduce(fa.part, fa.nparts, C, t.c0, sm, s, q);
    if (threadIdx.x < 64) {
        const int c = t.c0 + threadIdx.x;
        const BnChannel p = bn_params_from_sums(s, q, fa.count, fa.gamma[c], fa.beta[c], fa.eps);
        par[0][threadIdx.x] = p.sc; par[1][threadIdx.x] = p.sh;
        if (t.strip == 0) {
            bn_store_params(p, fa.bnp, C, c);
            if (fa.running_mean) bn_update_running(p, fa.count, fa.momentum, fa.running_mean[c], fa.running_var[c], fa.running_mean, fa.running_var, c);
        }
    }
    __syncthreads();
    float sc[8], sh[8], sc2[RES == RES_RAWBN ? 8 : 1], sh2[RES == RES_RAWBN ? 8 : 1];
    load_scale_shift<8>(&par[0][0], BNFIN_SLICE, t.j * 8, sc, sh);
    if constexpr (RES == RES_RAWBN) load_scale_shift<8>(res_bnp, C, t.c0 + t.j * 8, sc2, sh2);
    for (long p = (long)t.strip * 32 + t.pl; p < M; p += (long)t.nstrips * 32)
        bn_fwd_x3<8, RES>(p * C + t.c0 + t.j * 8, y, res, res_hi, res_lo, sc, sh, sc2, sh2, relu, out, hi, lo);
}

// BatchNorm backward, pass 2 with its finalize inside: part[nparts][C][2] = per-tile (sum dz, sum dz * xhat)
__global__ __launch_bounds__(256) void bn_fin_bwd_apply_x3_kernel(const float* __restrict__ part, int nparts, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, float* __restrict__ bwdp,
                                                                  const float* __restrict__ dout, const float* __restrict__ out,
                                                                  const float* __restrict__ y, const float* __restrict__ bnp, int C, long M,
                                                                  int relu, bf16_t* __restrict__ dy_hi, bf16_t* __restrict__ dy_lo,
                                                                  float* __restrict__ dz_out, const bf16_t* __restrict__ out_hi) {
    __shared__ double sm[4 * 64 * 2];
    __shared__ float par[2][BNFIN_SLICE];
    const BnFinTile t = bnfin_tile(C);
    double s, q; bnfin_reduce(part, nparts, C, t.c0, sm, s, q);
    if (threadIdx.x < 64) {
        par[0][threadIdx.x] = (float)s; par[1][threadIdx.x] = (float)q;
        if (t.strip == 0) bn_store_bwd_sums(s, q, dgamma, dbeta, bwdp, C, t.c0 + threadIdx.x);
    }
    __syncthreads();
    BnBwd<8> P; load_bwd_params<8>(P, bnp, C, t.c0 + t.j * 8, &par[0][0], BNFIN_SLICE, t.j * 8, 1.f / (float)M);
    for (long p = (long)t.strip * 32 + t.pl; p < M; p += (long)t.nstrips * 32)
        bn_bwd_x3(P, p * C + t.c0 + t.j * 8, dout, out, out_hi, y, relu, dy_hi, dy_lo, dz_out);
}

static bool bnfin_ok(int nparts, int C) {
    static const int on = getenv("AB_BNFIN_FUSE") ? atoi(getenv("AB_BNFIN_FUSE")) : 1;
    static const int maxrows = getenv("AB_BNFIN_ROWS") ? atoi(getenv("AB_BNFIN_ROWS")) : BNFIN_MAX_ROWS;
    return on && nparts > 0 && nparts <= maxrows && nparts <= BNFIN_MAX_ROWS && C % BNFIN_SLICE == 0;
}
// workgroups: every channel slice x enough pixel strips for ~4 workgroups per CU (each pays the prologue once)
static int bnfin_grid(long M, int C) {
    const int nsl = C / BNFIN_SLICE;
    long strips = (M + 31) / 32;
    const long want = (1024 + nsl - 1) / nsl;
    if (strips > want) strips = want;
    if (strips < 1) strips = 1;
    return (int)(strips * nsl);
}

// maxpool3x3/2(relu(bn(y))) forward of the split-bf16 path (the stem): maxpool_fwd_kernel<float>'s arithmetic and scan order with 8
// channels per thread and PFX_ROWS output rows per thread: consecutive output rows share an input row (2ho+1 = 2(ho+1)-1), which the
// one-row-per-workgroup version read twice (268 MB of input became ~400 MB of reads); here the bottom taps of a window are carried
// in registers as the top taps of the next -- six tap loads per output row instead of nine.
#define PFX_ROWS 4
__global__ __launch_bounds__(256) void maxpool_fwd_x3_kernel(const float* __restrict__ y, const float* __restrict__ bnp, int N, int H,
                                                             int W, int C, float* __restrict__ out, uint8_t* __restrict__ idx,
                                                             bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo,
                                                             float* __restrict__ ywin) {
    const int Ho = H / 2, Wo = W / 2, vc = C / 8;
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    if (col >= (unsigned)(Wo * vc)) return;
    const int wo = (int)(col / (unsigned)vc), cv = (int)(col - (unsigned)wo * vc);
    const int n = blockIdx.z, ho0 = blockIdx.y * PFX_ROWS;
    float sc[8], sh[8]; load_scale_shift<8>(bnp, C, cv * 8, sc, sh);
    const bool w0ok = wo > 0;                                // H, W even: only h = -1 / w = -1 can fall outside
    auto load_row = [&](int h, float (*r)[8]) {              // the three taps of input row h
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
            if (dw == 0 && !w0ok) continue;
            vload<float, 8>(y + (((long)n * H + h) * W + (wo * 2 + dw - 1)) * C + cv * 8, r[dw]);
        }
    };      // (RAW values are kept: relu(bn(.)) is applied at the comparison, so the winner's raw value is at hand for `ywin`)
    float top[3][8], mid[3][8], bot[3][8];
    if (ho0 > 0) load_row(ho0 * 2 - 1, top);
#pragma unroll
    for (int rr = 0; rr < PFX_ROWS; ++rr) {
        const int ho = ho0 + rr;
        if (ho >= Ho) break;
        load_row(ho * 2, mid);
        load_row(ho * 2 + 1, bot);
        float m[8], mraw[8]; uint32_t am[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { m[k] = -INFINITY; mraw[k] = 0.f; am[k] = 0; }
        auto scan = [&](const float (*r)[8], const int t0) {        // (inlined per row: the tap arrays stay in registers)
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                if (dw == 0 && !w0ok) continue;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float v = fmaxf(r[dw][k] * sc[k] + sh[k], 0.f);
                    if (v > m[k]) { m[k] = v; mraw[k] = r[dw][k]; am[k] = t0 + dw; }
                }
            }
        };
        if (ho > 0) scan(top, 0);
        scan(mid, 3);
        scan(bot, 6);
        const long e = ((((long)n * Ho + ho) * Wo + wo) * vc + cv) * 8;
        if (out) vstore<float, 8>(out + e, m);           // (NULL: the pooled tensor is wanted as planes only)
        pack_winners<8>(idx + e, am);
        store_split<8>(out_hi, out_lo, e, m);
        if (ywin) vstore<float, 8>(ywin + e, mraw);      // the winner's RAW conv output: what the backward's reduction needs of y
#pragma unroll
        for (int dw = 0; dw < 3; ++dw)
#pragma unroll
            for (int k = 0; k < 8; ++k) top[dw][k] = bot[dw][k];
    }
}

// Second half of maxpool3x3/2(relu(bn(y))) backward (pool_bwd_bn_reduce_kernel) for the split-bf16 path without the fp32 dz round trip: the same gather and mask again (winners + pooled gradient are
// a quarter of the map), then BatchNorm-backward pass 2 on the spot, dy written as planes.  Against (reduce writes dz, apply reads
// dz): 0.27 GB less written and 0.27 GB less read at the benchmark size for 84 MB of winners / pooled gradient read twice.
__global__ __launch_bounds__(256) void pool_bwd_bn_apply_x3_kernel(const uint8_t* __restrict__ idx, const float* __restrict__ dout,
                                                                    const float* __restrict__ y, const float* __restrict__ bnp,
                                                                    const float* __restrict__ bwdp, int N, int H, int W, int C,
                                                                    float invM, bf16_t* __restrict__ dy_hi, bf16_t* __restrict__ dy_lo) {
    const int Ho = H / 2, Wo = W / 2, vc = C / 8;
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    if (col >= (unsigned)(W * vc)) return;
    const int w = (int)(col / (unsigned)vc), cv = (int)(col - (unsigned)w * vc);
    const int n = blockIdx.z, p = blockIdx.y;
    float acc0[8], acc1[8], ya[8], yb[8], d0[8], d1[8];
    pool_gather_pair<float, 8>(idx, dout, n, p, w, Ho, Wo, C, cv * 8, acc0, acc1);
    const long e = ((((long)n * H + 2 * p) * W + w) * vc + cv) * 8;
    vload<float, 8>(y + e, ya);
    vload<float, 8>(y + e + (long)W * C, yb);
#pragma unroll
    for (int k = 0; k < 8; ++k) {      // channel by channel: a channel's six parameters are loaded where its two rows use them
        const int c = cv * 8 + k;
        BnBwd<1> P; load_bwd_params<1>(P, bnp, C, c, bwdp, C, c, invM);
        relu_mask<1>(P, RELU_RECOMPUTE, acc0 + k, nullptr, ya + k);
        relu_mask<1>(P, RELU_RECOMPUTE, acc1 + k, nullptr, yb + k);
        bn_bwd_dy<1>(P, acc0 + k, ya + k, d0 + k);
        bn_bwd_dy<1>(P, acc1 + k, yb + k, d1 + k);
    }
    store_split<8>(dy_hi, dy_lo, e, d0);
    store_split<8>(dy_hi, dy_lo, e + (long)W * C, d1);
}

// column sums of a split tensor (hi + lo): the bias gradient of the final layer from the dlogits planes
__global__ __launch_bounds__(256) void col_stats_x3_kernel(const bf16_t* __restrict__ hi, const bf16_t* __restrict__ lo, long M, int C,
                                                          int rows_per_block, float* __restrict__ part) {
    row_reduce<8>(M, C, C, 0, rows_per_block, part, [&](long r, int c, float* s, float* q) {
        float v[8]; load_planes<8>(hi, lo, r * C + c, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) { s[i] += v[i]; q[i] += v[i] * v[i]; }
    });
}

// BatchNorm-backward reduction of  maxpool3x3/2(relu(bn(y)))  over the POOLED elements only: the masked gradient is non-zero at
// window winners, so  sum dz = sum_w [relu'] dpool_w  and  sum dz*xhat = sum_w [relu'] dpool_w * xhat(ywin_w)  (an input position that
// wins several windows contributes once per window: the sums are linear).  Reads 2 x [N,H/2,W/2,C] fp32 instead of the full-resolution
// y + winners + pooled gradient; same mask expression as the forward.  part rows: ab_col_stats_nparts(N*H/2*W/2).
__global__ __launch_bounds__(256) void pool_win_bn_reduce_kernel(const float* __restrict__ dpool, const float* __restrict__ ywin,
                                                                  const float* __restrict__ bnp, long M, int C, int rows_per_block,
                                                                  float* __restrict__ part) {
    BnBwd<8> P; load_bn_stats<8>(P, bnp, C, row_lane_channel<8>(C));
    row_reduce<8>(M, C, C, 0, rows_per_block, part, [&](long r, int c, float* s, float* q) {
        float g[8], yw[8];
        vload<float, 8>(dpool + r * C + c, g);
        vload<float, 8>(ywin + r * C + c, yw);
        relu_mask<8>(P, RELU_RECOMPUTE, g, nullptr, yw);
        bn_bwd_sums<8>(P, g, yw, s, q);
    });
}

// ================================================================ C ABI
static inline int grid_for(long nvec) { long b = (nvec + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }
static inline int vec_of(int dtype) { return dtype == AB_DT_F32 ? 4 : 8; }      // elements per 16-byte vector
// runs the statement(s) with T = float / bf16_t for dtype; any other dtype returns AB_EINVAL
#define DISPATCH(dtype, ...) do { \
        if ((dtype) == AB_DT_F32) { using T = float; __VA_ARGS__; } \
        else if ((dtype) == AB_DT_BF16) { using T = bf16_t; __VA_ARGS__; } \
        else return AB_EINVAL; \
    } while (0)
// the finalize launches: launch(CPW as an integral constant, grid) for the CPW that finalize_cpw() picks
template <typename F> static void launch_finalize(int C, F launch) {
    switch (finalize_cpw()) {
    case 2: launch(std::integral_constant<int, 2>(), (C + 1) / 2); break;
    case 4: launch(std::integral_constant<int, 4>(), (C + 3) / 4); break;
    default: launch(std::integral_constant<int, 8>(), (C + 7) / 8); break;
    }
}
// grid of the pooling kernels: x = 256-thread workgroups over a row's cols x vc channel vectors, y = rows, z = N
static inline dim3 pool_grid(int cols, int vc, int rows, int N) { return dim3((unsigned)(((long)cols * vc + 255) / 256), (unsigned)rows, (unsigned)N); }

extern "C" int ab_col_stats_nparts(long M) { int r = red_rows(M); return (int)((M + r - 1) / r); }

extern "C" int ab_col_stats(const void* x, int dtype, long M, int C, float* part, void* stream) {
    if (!x || !part) return AB_EINVAL;
    int V = vec_of(dtype);
    if (C % V || C / V > 256) return AB_ESHAPE;
    int np = ab_col_stats_nparts(M); int rl = 256 / (C / V); size_t sh = (size_t)rl * C * 2 * 4;
    DISPATCH(dtype, col_stats_kernel<T><<<np, 256, sh, as_stream(stream)>>>((const T*)x, M, C, red_rows(M), part));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_bn_finalize(const float* part, int nparts, int C, long count, const float* gamma, const float* beta,
                              float eps, float momentum, float* running_mean, float* running_var, float* bnp,
                              void* stream) {
    if (!part || !gamma || !beta || !bnp) return AB_EINVAL;
    hipStream_t st = as_stream(stream);
    launch_finalize(C, [&](auto cpw, int grid) {
        bn_finalize_kernel<decltype(cpw)::value><<<grid, 1024, 0, st>>>(part, nparts, C, count, gamma, beta, eps, momentum, running_mean, running_var, bnp);
    });
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_bn_eval_params(int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                 float eps, float* bnp, void* stream) {
    if (!gamma || !beta || !rm || !rv || !bnp) return AB_EINVAL;
    bn_eval_params_kernel<<<(C + 255) / 256, 256, 0, as_stream(stream)>>>(C, gamma, beta, rm, rv, eps, bnp);
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_bn_eval_params_batch(const float* flat, const float* stats, const int32_t* desc_dev, int n, int max_c, float eps,
                                       float* out, void* stream) {
    if (!flat || !stats || !desc_dev || !out) return AB_EINVAL;
    if (n <= 0 || max_c <= 0) return AB_ESHAPE;
    bn_eval_params_batch_kernel<<<dim3((max_c + 255) / 256, n), 256, 0, as_stream(stream)>>>(flat, stats, (const int*)desc_dev, eps, out);
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_bn_apply(const void* y, const void* res, const float* bnp, int dtype, long M, int C, int relu,
                           void* out, void* stream) {
    if (!y || !bnp || !out) return AB_EINVAL;
    int V = vec_of(dtype); if (C % V) return AB_ESHAPE;
    long nvec = M * C / V;
    DISPATCH(dtype, bn_apply_kernel<T><<<grid_for(nvec), 256, 0, as_stream(stream)>>>((const T*)y, (const T*)res, bnp, nvec, C, relu, (T*)out));
    AB_LAUNCH_CHECK(); return 0;
}

static void launch_bn_bwd_finalize(const float* part, int np, int C, float* dgamma, float* dbeta, float* bwdp, hipStream_t st) {
    launch_finalize(C, [&](auto cpw, int grid) { bn_bwd_finalize_kernel<decltype(cpw)::value><<<grid, 1024, 0, st>>>(part, np, C, dgamma, dbeta, bwdp); });
}

static int bn_bwd_impl(const void* dout, const void* out, const void* y, const float* bnp, int dtype, long M, int C,
                       int relu, float* part, float* bwdp, float* dgamma, float* dbeta, void* dy, void* dz_out,
                       const uint8_t* pool_idx, int pH, int pW, hipStream_t st, int given_parts = 0) {
    int V = vec_of(dtype);
    int ysl = 1;                                  // channel slices of the reduction (<= 256 V-channel groups each)
    while (C / V / ysl > 256) ysl *= 2;
    if (C % V || C % (V * ysl)) return AB_ESHAPE;
    int np = given_parts > 0 ? given_parts : ab_col_stats_nparts(M); const int cs = C / ysl; int rl = 256 / (cs / V); size_t sh = (size_t)rl * cs * 2 * 4;
    if (given_parts <= 0)
        DISPATCH(dtype, bn_bwd_reduce_kernel<T><<<dim3(np, ysl), 256, sh, st>>>((const T*)dout, (const T*)out, (const T*)y, bnp, M, C, relu,
                                                                                red_rows(M), part, pool_idx, pH, pW));
    AB_LAUNCH_CHECK();
    launch_bn_bwd_finalize(part, np, C, dgamma, dbeta, bwdp, st);
    AB_LAUNCH_CHECK();
    long nvec = M * C / V;
    DISPATCH(dtype, bn_bwd_apply_kernel<T><<<grid_for(nvec), 256, 0, st>>>((const T*)dout, (const T*)out, (const T*)y, bnp, bwdp, nvec, C, M, relu,
                                                                           (T*)dy, (T*)dz_out, pool_idx, pH, pW));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_bn_bwd(const void* dout, const void* out, const void* y, const float* bnp, int dtype, long M, int C,
                         int relu, float* part, float* bwdp, float* dgamma, float* dbeta, void* dy, void* dz_out,
                         void* stream) {
    if (!dout || !y || !bnp || !part || !bwdp || !dgamma || !dbeta || !dy || (relu == 1 && !out) || relu < 0 || relu > 2) return AB_EINVAL;
    return bn_bwd_impl(dout, out, y, bnp, dtype, M, C, relu, part, bwdp, dgamma, dbeta, dy, dz_out, nullptr, 0, 0, as_stream(stream));
}

// Second half of ab_bn_bwd only (finalize + apply): `part` [nparts][C][2] already holds the per-tile sums (sum dz,
// sum dz*xhat), written by ab_conv2d_dgrad_bnstats.
extern "C" int ab_bn_bwd_apply(const void* dout, const void* out, const void* y, const float* bnp, int dtype, long M, int C,
                               int relu, const float* part, int nparts, float* bwdp, float* dgamma, float* dbeta, void* dy,
                               void* dz_out, void* stream) {
    if (!dout || !y || !bnp || !part || nparts < 1 || !bwdp || !dgamma || !dbeta || !dy || (relu == 1 && !out) || relu < 0 || relu > 2) return AB_EINVAL;
    return bn_bwd_impl(dout, out, y, bnp, dtype, M, C, relu, (float*)part, bwdp, dgamma, dbeta, dy, dz_out, nullptr, 0, 0,
                       as_stream(stream), nparts);
}

// Backward of  maxpool3x3/2( relu( bn(y) ) )  in the two BN passes: the pooled gradient dpool [N,H/2,W/2,C] is scattered
// on the fly through the recorded winners (idx of ab_bn_relu_maxpool3x3s2_fwd), the ReLU mask is recomputed from y.
extern "C" int ab_bn_relu_maxpool_bwd(const void* dpool, const void* idx, const void* y, const float* bnp, int dtype, int N,
                                      int H, int W, int C, float* part, float* bwdp, float* dgamma, float* dbeta, void* dy,
                                      void* stream) {
    if (!dpool || !idx || !y || !bnp || !part || !bwdp || !dgamma || !dbeta || !dy) return AB_EINVAL;
    if ((H & 1) || (W & 1)) return AB_ESHAPE;
    return bn_bwd_impl(dpool, nullptr, y, bnp, dtype, (long)N * H * W, C, 2, part, bwdp, dgamma, dbeta, dy, nullptr,
                       (const uint8_t*)idx, H, W, as_stream(stream));
}

extern "C" int ab_add(const void* a, const void* b, int dtype, long n, void* out, void* stream) {
    int V = vec_of(dtype); if (n % V) return AB_ESHAPE;
    long nvec = n / V;
    DISPATCH(dtype, add_kernel<T><<<grid_for(nvec), 256, 0, as_stream(stream)>>>((const T*)a, (const T*)b, nvec, (T*)out));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_maxpool3x3s2_fwd(const void* x, int dtype, int N, int H, int W, int C, void* out, void* idx, void* stream) {
    int V = vec_of(dtype); if (C % V || (H & 1) || (W & 1)) return AB_ESHAPE;
    DISPATCH(dtype, maxpool_fwd_kernel<T><<<pool_grid(W / 2, C / V, H / 2, N), 256, 0, as_stream(stream)>>>((const T*)x, nullptr, N, H, W, C, (T*)out,
                                                                                                            (uint8_t*)idx));
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_bn_relu_maxpool3x3s2_fwd(const void* y, const float* bnp, int dtype, int N, int H, int W, int C, void* out,
                                           void* idx, void* stream) {
    if (!y || !bnp || !out) return AB_EINVAL;
    int V = vec_of(dtype); if (C % V || (H & 1) || (W & 1)) return AB_ESHAPE;
    DISPATCH(dtype, maxpool_fwd_kernel<T><<<pool_grid(W / 2, C / V, H / 2, N), 256, 0, as_stream(stream)>>>((const T*)y, bnp, N, H, W, C, (T*)out,
                                                                                                            (uint8_t*)idx));
    AB_LAUNCH_CHECK(); return 0;
}
// fp32 in, fp32 + (hi, lo) bf16 planes out: the pooled tensor is read by three split-bf16 convolutions (layer1.0 conv1, its
// weight gradient, the residual stays fp32)
extern "C" int ab_bn_relu_maxpool3x3s2_fwd_x3(const float* y, const float* bnp, int N, int H, int W, int C, float* out, void* out_hi,
                                              void* out_lo, void* idx, void* stream) {
    if (!y || !bnp || !out || !out_hi || !out_lo) return AB_EINVAL;
    if (C % 4 || (H & 1) || (W & 1)) return AB_ESHAPE;
    static const int v8 = getenv("AB_POOL_FWD_V8") ? atoi(getenv("AB_POOL_FWD_V8")) : 1;
    if (v8 && C % 8 == 0 && idx) {
        const dim3 g8 = pool_grid(W / 2, C / 8, (H / 2 + PFX_ROWS - 1) / PFX_ROWS, N);
        maxpool_fwd_x3_kernel<<<g8, 256, 0, as_stream(stream)>>>(y, bnp, N, H, W, C, out, (uint8_t*)idx, (bf16_t*)out_hi, (bf16_t*)out_lo, nullptr);
        AB_LAUNCH_CHECK(); return 0;
    }
    const dim3 g4 = pool_grid(W / 2, C / 4, H / 2, N);
    maxpool_fwd_kernel<float><<<g4, 256, 0, as_stream(stream)>>>(y, bnp, N, H, W, C, out, (uint8_t*)idx, (bf16_t*)out_hi, (bf16_t*)out_lo);
    AB_LAUNCH_CHECK(); return 0;
}
// ... also writing ywin [N,H/2,W/2,C] fp32: the RAW conv output at each window's winner, for ab_bn_relu_maxpool_bwd_x3w
extern "C" int ab_bn_relu_maxpool3x3s2_fwd_x3w(const float* y, const float* bnp, int N, int H, int W, int C, float* out, void* out_hi,
                                               void* out_lo, void* idx, float* ywin, void* stream) {
    if (!y || !bnp || !out_hi || !out_lo || !idx || !ywin) return AB_EINVAL;          // out may be NULL: planes only
    if (C % 8 || (H & 1) || (W & 1)) return AB_ESHAPE;
    const dim3 g8 = pool_grid(W / 2, C / 8, (H / 2 + PFX_ROWS - 1) / PFX_ROWS, N);
    maxpool_fwd_x3_kernel<<<g8, 256, 0, as_stream(stream)>>>(y, bnp, N, H, W, C, out, (uint8_t*)idx, (bf16_t*)out_hi, (bf16_t*)out_lo, ywin);
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_maxpool3x3s2_bwd(const void* idx, const void* dout, int dtype, int N, int H, int W, int C, void* dx,
                                   void* stream) {
    int V = vec_of(dtype); if (C % V || (H & 1) || (W & 1)) return AB_ESHAPE;
    DISPATCH(dtype, maxpool_bwd_kernel<T><<<pool_grid(W, C / V, H / 2, N), 256, 0, as_stream(stream)>>>((const uint8_t*)idx, (const T*)dout, N, H, W, C,
                                                                                                    (T*)dx));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_avgpool_fwd(const void* x, int dtype, int N, int HW, int C, float* out, void* stream) {
    if (!x || !out) return AB_EINVAL;
    const int V = vec_of(dtype); if (C % V) return AB_ESHAPE;
    DISPATCH(dtype, avgpool_fwd_kernel<T><<<dim3(N, (C + 32 * V - 1) / (32 * V)), 256, 0, as_stream(stream)>>>((const T*)x, HW, C, out));
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_avgpool_bwd(const float* g, int dtype, int N, int HW, int C, void* dx, int accumulate, void* stream) {
    if (!g || !dx) return AB_EINVAL;
    const int V = vec_of(dtype); if (C % V) return AB_ESHAPE;
    const long nvec = (long)N * HW * C / V;
    DISPATCH(dtype, avgpool_bwd_kernel<T><<<grid_for(nvec), 256, 0, as_stream(stream)>>>(g, HW, C, nvec, (T*)dx, accumulate));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_cast_f32_bf16(const float* src, long n, void* dst, void* stream) {
    cast_f32_bf16_kernel<<<grid_for(n), 256, 0, as_stream(stream)>>>(src, n, (bf16_t*)dst);
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_transpose_oki(const float* src, int O, int K, int I, int dtype, void* dst, void* stream) {
    long n = (long)O * K * I;
    DISPATCH(dtype, transpose_oki_kernel<T><<<grid_for(n), 256, 0, as_stream(stream)>>>(src, O, K, I, (T*)dst));
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_transpose_oki_batch(const ab_transpose_desc* desc_dev, int ntensors, long total_tiles, int dtype,
                                      void* stream) {
    if (!desc_dev || ntensors < 1 || total_tiles < 1 || total_tiles > 0x7fffffffL) return AB_EINVAL;
    DISPATCH(dtype, transpose_oki_batch_kernel<T><<<(unsigned)total_tiles, 256, 0, as_stream(stream)>>>(desc_dev, ntensors));
    AB_LAUNCH_CHECK(); return 0;
}
extern "C" int ab_image_pad_nhwc4(const float* img_nchw, int dtype, int N, int H, int W, void* out, void* stream) {
    long n = (long)N * (H + 6) * (W + 8);
    DISPATCH(dtype, image_pad_kernel<T><<<grid_for(n), 256, 0, as_stream(stream)>>>(img_nchw, N, H, W, (T*)out));
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_relu_bwd(const void* dout, const void* out, int dtype, long n, void* dz, void* stream) {
    int V = vec_of(dtype); if (n % V) return AB_ESHAPE;
    long nvec = n / V;
    DISPATCH(dtype, relu_bwd_kernel<T><<<grid_for(nvec), 256, 0, as_stream(stream)>>>((const T*)dout, (const T*)out, nvec, (T*)dz));
    AB_LAUNCH_CHECK(); return 0;
}
// column sums (bias gradient) of x [M][C]: part = float [ab_col_stats_nparts(M)][C][2] workspace, out float [C]
extern "C" int ab_col_sum(const void* x, int dtype, long M, int C, float* part, float* out, void* stream) {
    int rc = ab_col_stats(x, dtype, M, C, part, stream);
    if (rc) return rc;
    colsum_finalize_kernel<<<(C + 7) / 8, 256, 0, as_stream(stream)>>>(part, ab_col_stats_nparts(M), C, out);
    AB_LAUNCH_CHECK(); return 0;
}

// ---- split-bf16 producers (fp32 in; see the kernels above).  out (bn_apply) / dz_out may be NULL.
extern "C" int ab_bn_apply_x3(const float* y, const float* res, const float* bnp, long M, int C, int relu, float* out,
                              void* out_hi, void* out_lo, void* stream) {
    if (!y || !bnp || !out_hi || !out_lo) return AB_EINVAL;
    if (C % 8 == 4) {
        bn_apply_x3_c4_kernel<<<grid_for(M * C / 4), 256, 0, as_stream(stream)>>>(y, res, bnp, M * C / 4, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo,
                                                                                  nullptr, nullptr);
        AB_LAUNCH_CHECK(); return 0;
    }
    if (C % 8) return AB_ESHAPE;
    const long nvec = M * C / 8;
    bn_apply_x3_kernel<false><<<grid_for(nvec), 256, 0, as_stream(stream)>>>(y, res, bnp, nvec, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo);
    AB_LAUNCH_CHECK(); return 0;
}

// ... with the residual given as the raw output of the downsample conv + its BatchNorm parameters
extern "C" int ab_bn_apply_x3_resbn(const float* y, const float* res_y, const float* bnp, const float* res_bnp, long M, int C,
                                    int relu, float* out, void* out_hi, void* out_lo, void* stream) {
    if (!y || !res_y || !bnp || !res_bnp || !out_hi || !out_lo) return AB_EINVAL;
    if (C % 8) return AB_ESHAPE;
    const long nvec = M * C / 8;
    bn_apply_x3_kernel<true><<<grid_for(nvec), 256, 0, as_stream(stream)>>>(y, res_y, bnp, nvec, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo, res_bnp);
    AB_LAUNCH_CHECK(); return 0;
}

// ... with the residual given as its (hi, lo) planes
extern "C" int ab_bn_apply_x3_respl(const float* y, const void* res_hi, const void* res_lo, const float* bnp, long M, int C, int relu,
                                    float* out, void* out_hi, void* out_lo, void* stream) {
    if (!y || !res_hi || !res_lo || !bnp || !out_hi || !out_lo) return AB_EINVAL;
    if (C % 8 == 4) {
        bn_apply_x3_c4_kernel<<<grid_for(M * C / 4), 256, 0, as_stream(stream)>>>(y, nullptr, bnp, M * C / 4, C, relu, out, (bf16_t*)out_hi,
                                                                                  (bf16_t*)out_lo, (const bf16_t*)res_hi, (const bf16_t*)res_lo);
        AB_LAUNCH_CHECK(); return 0;
    }
    if (C % 8) return AB_ESHAPE;
    const long nvec = M * C / 8;
    bn_apply_x3_kernel<false, true><<<grid_for(nvec), 256, 0, as_stream(stream)>>>(y, nullptr, bnp, nvec, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo,
                                                                                 nullptr, (const bf16_t*)res_hi, (const bf16_t*)res_lo);
    AB_LAUNCH_CHECK(); return 0;
}

// BatchNorm finalize + apply in ONE launch (training forward): part [nparts][C][2] are the per-tile (sum, sum of squares) a convolution's
// epilogue left, count = elements per channel; writes bnp [4][C] and updates the running statistics like ab_bn_finalize, then applies like
// ab_bn_apply_x3 / _respl (res_hi != NULL) / _resbn (res_bnp != NULL).  AB_ESHAPE when the shape is not taken (nparts > 64 or C % 64:
// ab_bn_fin_apply_x3_ok says so beforehand) -- the caller then runs ab_bn_finalize + ab_bn_apply_x3*.
extern "C" int ab_bn_fin_apply_x3_ok(int nparts, int C) { return bnfin_ok(nparts, C) ? 1 : 0; }

extern "C" int ab_bn_fin_apply_x3(const float* part, int nparts, long count, const float* gamma, const float* beta, float eps, float momentum,
                                  float* running_mean, float* running_var, float* bnp, const float* y, const float* res,
                                  const void* res_hi, const void* res_lo, const float* res_bnp, long M, int C, int relu, float* out,
                                  void* out_hi, void* out_lo, void* stream) {
    if (!part || !gamma || !beta || !bnp || !y || !out_hi || !out_lo || (!res_hi != !res_lo) || (res_bnp && !res) || (res_hi && (res || res_bnp)))
        return AB_EINVAL;
    if (!bnfin_ok(nparts, C)) return AB_ESHAPE;
    BnFinArgs fa = {part, nparts, count, gamma, beta, eps, momentum, running_mean, running_var, bnp};
    const int grid = bnfin_grid(M, C);
    hipStream_t st = as_stream(stream);
    if (res_hi) bn_fin_apply_x3_kernel<1><<<grid, 256, 0, st>>>(fa, y, nullptr, (const bf16_t*)res_hi, (const bf16_t*)res_lo, nullptr, M, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo);
    else if (res_bnp) bn_fin_apply_x3_kernel<2><<<grid, 256, 0, st>>>(fa, y, res, nullptr, nullptr, res_bnp, M, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo);
    else bn_fin_apply_x3_kernel<0><<<grid, 256, 0, st>>>(fa, y, res, nullptr, nullptr, nullptr, M, C, relu, out, (bf16_t*)out_hi, (bf16_t*)out_lo);
    AB_LAUNCH_CHECK(); return 0;
}

// ab_bn_bwd / ab_bn_bwd_apply with dy as split planes: nparts_given = 0 runs the reduction pass into `part`
// ([ab_col_stats_nparts(M)][C][2]); > 0 takes `part` as already reduced per-tile sums (see ab_bn_bwd_apply).
extern "C" int ab_bn_bwd_x3(const float* dout, const void* out, int out_is_hi_plane, const float* y, const float* bnp, long M, int C,
                            int relu, float* part, int nparts_given, float* bwdp, float* dgamma, float* dbeta, void* dy_hi,
                            void* dy_lo, float* dz_out, void* stream) {
    if (!dout || !y || !bnp || !part || !bwdp || !dgamma || !dbeta || !dy_hi || !dy_lo || (relu == 1 && !out) || relu < 0 || relu > 2)
        return AB_EINVAL;
    const float* out_f = out_is_hi_plane ? nullptr : (const float*)out;
    const bf16_t* out_h = out_is_hi_plane ? (const bf16_t*)out : nullptr;
    int ysl = 1;                                  // channel slices of the reduction (<= 256 four-channel groups each)
    while (C / 4 / ysl > 256) ysl *= 2;
    if (C % 8 || C % (4 * ysl)) return AB_ESHAPE;
    hipStream_t st = as_stream(stream);
    int np = nparts_given > 0 ? nparts_given : ab_col_stats_nparts(M);
    if (nparts_given <= 0) {
        const int cs = C / ysl, rl = 256 / (cs / 4); const size_t sh = (size_t)rl * cs * 2 * 4;
        bn_bwd_reduce_kernel<float><<<dim3(np, ysl), 256, sh, st>>>(dout, out_f, y, bnp, M, C, relu, red_rows(M), part, nullptr, 0, 0, out_h);
        AB_LAUNCH_CHECK();
    }
    if (bnfin_ok(np, C)) {          // few partial rows: the apply pass reduces them itself (no finalize launch)
        bn_fin_bwd_apply_x3_kernel<<<bnfin_grid(M, C), 256, 0, st>>>(part, np, dgamma, dbeta, bwdp, dout, out_f, y, bnp, C, M, relu, (bf16_t*)dy_hi,
                                                                     (bf16_t*)dy_lo, dz_out, out_h);
        AB_LAUNCH_CHECK(); return 0;
    }
    launch_bn_bwd_finalize(part, np, C, dgamma, dbeta, bwdp, st);
    AB_LAUNCH_CHECK();
    const long nvec = M * C / 8;
    bn_bwd_apply_x3_kernel<<<grid_for(nvec), 256, 0, st>>>(dout, out_f, y, bnp, bwdp, nvec, C, M, relu, (bf16_t*)dy_hi, (bf16_t*)dy_lo, dz_out, out_h);
    AB_LAUNCH_CHECK(); return 0;
}

// Backward of  maxpool3x3/2( relu( bn(y) ) )  for the split-bf16 path (resnet.py:154-157 backwards; the stem).  One pass scatters
// the pooled gradient to the full resolution, masks it and reduces it (pool_bwd_bn_reduce_kernel, part rows =
// ab_bn_relu_maxpool_bwd_x3_nparts); finalize; the apply pass repeats the gather and writes dy as planes (pool_bwd_bn_apply_x3_kernel;
// AB_POOL_BWD_REGATHER=0: the reduce pass stores the masked gradient in the fp32 scratch `dz` and the generic apply pass reads it).
// row pairs per workgroup of the reduction: 4 / 8 / 16 -> 91 + 18 / 92 + 9 / 110 + 6 us for the pass + its finalize over 2 048 / 1 024 /
// 512 partial rows
static int pbr_rp() { static const int v = getenv("AB_PBR_RP") ? atoi(getenv("AB_PBR_RP")) : 8; return (v == 4 || v == 16) ? v : 8; }
static dim3 pbr_grid(int N, int H, int W, int C) { return pool_grid(W, C / 4, (H / 2 + pbr_rp() - 1) / pbr_rp(), N); }
extern "C" int ab_bn_relu_maxpool_bwd_x3_nparts(int N, int H, int W, int C) {
    if ((H & 1) || (W & 1) || C % 8 || C / 4 > 256 || 256 % (C / 4)) return 0;
    const dim3 g = pbr_grid(N, H, W, C);
    return (int)(g.x * g.y * g.z);
}
extern "C" int ab_bn_relu_maxpool_bwd_x3(const float* dpool, const void* idx, const float* y, const float* bnp, int N, int H, int W,
                                         int C, float* part, float* bwdp, float* dgamma, float* dbeta, float* dz, void* dy_hi,
                                         void* dy_lo, void* stream) {
    if (!dpool || !idx || !y || !bnp || !part || !bwdp || !dgamma || !dbeta || !dz || !dy_hi || !dy_lo) return AB_EINVAL;
    const int np = ab_bn_relu_maxpool_bwd_x3_nparts(N, H, W, C);
    if (!np) return AB_ESHAPE;
    hipStream_t st = as_stream(stream);
    const dim3 grid = pbr_grid(N, H, W, C);
    static const int regather = getenv("AB_POOL_BWD_REGATHER") ? atoi(getenv("AB_POOL_BWD_REGATHER")) : 1;
    const long M = (long)N * H * W, nvec = M * C / 8;
#define PBR_LAUNCH(RP, WR) pool_bwd_bn_reduce_kernel<RP, WR><<<grid, 256, 256 * 8 * 4, st>>>((const uint8_t*)idx, dpool, y, bnp, N, H, W, C, dz, part)
    const int rp = pbr_rp();
    if (regather) { if (rp == 4) PBR_LAUNCH(4, false); else if (rp == 8) PBR_LAUNCH(8, false); else PBR_LAUNCH(16, false); }
    else { if (rp == 4) PBR_LAUNCH(4, true); else if (rp == 8) PBR_LAUNCH(8, true); else PBR_LAUNCH(16, true); }
#undef PBR_LAUNCH
    AB_LAUNCH_CHECK();
    launch_bn_bwd_finalize(part, np, C, dgamma, dbeta, bwdp, st);
    AB_LAUNCH_CHECK();
    if (regather) {
        pool_bwd_bn_apply_x3_kernel<<<pool_grid(W, C / 8, H / 2, N), 256, 0, st>>>((const uint8_t*)idx, dpool, y, bnp, bwdp, N, H, W, C, 1.f / (float)M,
                                                       (bf16_t*)dy_hi, (bf16_t*)dy_lo);
    } else
        bn_bwd_apply_x3_kernel<<<grid_for(nvec), 256, 0, st>>>(dz, nullptr, y, bnp, bwdp, nvec, C, M, 0, (bf16_t*)dy_hi, (bf16_t*)dy_lo, nullptr, nullptr);
    AB_LAUNCH_CHECK(); return 0;
}

// ab_bn_relu_maxpool_bwd_x3 with the reduction over the pooled elements (pool_win_bn_reduce_kernel: dpool + ywin, 134 MB at the
// benchmark size instead of 352); part: ab_col_stats_nparts(N*H/2*W/2) rows.
extern "C" int ab_bn_relu_maxpool_bwd_x3w(const float* dpool, const void* idx, const float* ywin, const float* y, const float* bnp,
                                          int N, int H, int W, int C, float* part, float* bwdp, float* dgamma, float* dbeta,
                                          void* dy_hi, void* dy_lo, void* stream) {
    if (!dpool || !idx || !ywin || !y || !bnp || !part || !bwdp || !dgamma || !dbeta || !dy_hi || !dy_lo) return AB_EINVAL;
    if ((H & 1) || (W & 1) || C % 8 || C / 8 > 256) return AB_ESHAPE;
    hipStream_t st = as_stream(stream);
    const long Mp = (long)N * (H / 2) * (W / 2), M = (long)N * H * W;
    const int np = ab_col_stats_nparts(Mp), rl = 256 / (C / 8);
    pool_win_bn_reduce_kernel<<<np, 256, (size_t)rl * C * 2 * 4, st>>>(dpool, ywin, bnp, Mp, C, red_rows(Mp), part);
    AB_LAUNCH_CHECK();
    launch_bn_bwd_finalize(part, np, C, dgamma, dbeta, bwdp, st);
    AB_LAUNCH_CHECK();
    pool_bwd_bn_apply_x3_kernel<<<pool_grid(W, C / 8, H / 2, N), 256, 0, st>>>((const uint8_t*)idx, dpool, y, bnp, bwdp, N, H, W, C, 1.f / (float)M,
                                                   (bf16_t*)dy_hi, (bf16_t*)dy_lo);
    AB_LAUNCH_CHECK(); return 0;
}

// ab_transpose_oki_batch with bf16 outputs as split planes: hi at desc.dst, lo at desc.dst + lo_offset_elems
extern "C" int ab_transpose_oki_batch_x3(const ab_transpose_desc* desc_dev, int ntensors, long total_tiles, long lo_offset_elems,
                                         void* stream) {
    if (!desc_dev || ntensors < 1 || total_tiles < 1 || total_tiles > 0x7fffffffL || lo_offset_elems <= 0) return AB_EINVAL;
    transpose_oki_batch_kernel<bf16_t><<<(unsigned)total_tiles, 256, 0, as_stream(stream)>>>(desc_dev, ntensors, lo_offset_elems);
    AB_LAUNCH_CHECK(); return 0;
}

// ab_col_sum over a split tensor (planes hi, lo: bf16 [M][C]); part as in ab_col_sum
extern "C" int ab_col_sum_x3(const void* hi, const void* lo, long M, int C, float* part, float* out, void* stream) {
    if (!hi || !lo || !part || !out) return AB_EINVAL;
    if (C % 8 || C / 8 > 256) return AB_ESHAPE;
    const int np = ab_col_stats_nparts(M), rl = 256 / (C / 8);
    col_stats_x3_kernel<<<np, 256, (size_t)rl * C * 2 * 4, as_stream(stream)>>>((const bf16_t*)hi, (const bf16_t*)lo, M, C, red_rows(M), part);
    AB_LAUNCH_CHECK();
    colsum_finalize_kernel<<<(C + 7) / 8, 256, 0, as_stream(stream)>>>(part, np, C, out);
    AB_LAUNCH_CHECK(); return 0;
}
