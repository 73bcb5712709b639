// Head of the projection discriminator ("cGANs with Projection Discriminator"): plane sums of the trunk's feature map, the rating's
// inner product with them and the 1x1 / padding 1 convolution psi, forward and backward.
//
// Replaces, in the reference (NLayerProjectionDiscriminator.forward, proj=True),
//   h = torch.sum(self.phi(input), dim=(2, 3), keepdim=True)                                  models/networks.py:830
//   w_y = self.l_y(y)                                                                         models/networks.py:831
//   output = torch.sum(h * w_y, dim=1, keepdim=True) + self.psi(h)                            models/networks.py:832
//   torch.sigmoid(output) if self._sigm                                                       models/networks.py:838
// and autograd's backward through these lines.
//
// Bandwidth-bound: the forward pass reads p once, the backward pass writes dp once.  A workgroup of the two plane kernels owns
// PH_PLANES consecutive (b, c) planes -- one contiguous block of PH_PLANES * HW elements whose start is 16-byte aligned whenever the
// tensor is (PH_PLANES * HW * sizeof(T) is a multiple of 16 for both storage types) -- and walks it 16 bytes per thread and step,
// whatever HW is: a 16-byte piece may straddle planes (HW = 49, 225, 961 ...), every element is filed under its own plane.  A tensor
// that is only element-aligned takes the same walk with element accesses: the same thread handles the same elements in the same
// order, so both paths give the same bits.  Every sum runs in a fixed order in float64 and is rounded once; no float atomics; results
// are bit-identical from run to run and beside other streams' work.  Two launches per direction: the second consumes what the
// first left in h (forward) or in the caller's workspace (backward).
#include "common.h"

namespace pcgan {

static constexpr int PH_THREADS = 256;
static constexpr int PH_WAVES = PH_THREADS / 64;
static constexpr int PH_PLANES = 8;            // planes per workgroup: 2048 workgroups at B = 32, C = 512 (8 per CU on 256 CUs)
static constexpr int PH_MAX_NZ = 16;
static constexpr int PH_MAX_HW = 1 << 27;      // PH_PLANES * HW stays below 2^31

template <typename T> struct PhVec;
template <> struct PhVec<float> { static constexpr int N = 4; };
template <> struct PhVec<bf16> { static constexpr int N = 8; };

// N consecutive elements starting at p as floats: one 16-byte access (vec) or N element accesses
__device__ __forceinline__ void ph_load(const float* p, float (&v)[4], int vec) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = p[i];
    }
}
__device__ __forceinline__ void ph_load(const bf16* p, float (&v)[8], int vec) {
    if (vec) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(u[i] << 16);
            v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)p[i];
    }
}
__device__ __forceinline__ void ph_store(float* p, const float (&v)[4], int vec) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = v[i];
    }
}
__device__ __forceinline__ void ph_store(bf16* p, const float (&v)[8], int vec) {
    typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
    if (vec) {
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (bf16)v[i];
        *reinterpret_cast<bf16x8*>(p) = o;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = (bf16)v[i];
    }
}

// ---- forward, launch 1: h[plane] = sum of the plane -------------------------------------------------------------------------------
// A thread's elements ascend, so the plane they belong to never decreases: it keeps one running sum, and files it in its own column of
// part[plane][thread] when the plane changes (each slot is written at most once; the others stay 0).  A plane's sum is then the sum of
// its row in thread order.
template <typename T>
__global__ void __launch_bounds__(PH_THREADS) proj_plane_sum_kernel(const T* __restrict__ p, float* __restrict__ h, int planes, int HW,
                                                                    int vec) {
    constexpr int V = PhVec<T>::N;
    __shared__ double part[PH_PLANES][PH_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane0 = blockIdx.x * PH_PLANES;
    const int np = min(PH_PLANES, planes - plane0);
    const int total = np * HW;                       // elements of this workgroup's block
    const T* base = p + (size_t)plane0 * HW;
#pragma unroll
    for (int j = 0; j < PH_PLANES; ++j) part[j][tid] = 0.0;
    int pl = -1;
    double acc = 0.0;
    for (int o = tid * V; o < total; o += PH_THREADS * V) {
        float v[V];
        const int n = min(V, total - o);
        if (n == V) {
            ph_load(base + o, v, vec);
        } else {                                     // the ragged end of the tensor's last block
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = i < n ? (float)base[o + i] : 0.f;
        }
        int q = o / HW, r = o - q * HW;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (i < n) {
                if (q != pl) {
                    if (pl >= 0) part[pl][tid] = acc;
                    pl = q;
                    acc = 0.0;
                }
                acc += (double)v[i];
                if (++r == HW) { r = 0; ++q; }
            }
        }
    }
    if (pl >= 0) part[pl][tid] = acc;
    __syncthreads();
    for (int j = wave; j < np; j += PH_WAVES) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PH_THREADS / 64; ++k) s += part[j][lane + 64 * k];
        s = wave_sum_d(s);
        if (lane == 0) h[plane0 + j] = (float)s;
    }
}

struct ProjRowArgs {
    const float *h, *y, *psi_w, *psi_b, *ly_w, *ly_b;
    int B, C, nz, By, sigmoid;
};

// wy[b][c] = sum_j l_y.weight[c][j] y[b][j] + l_y.bias[c]
__device__ __forceinline__ double ph_wy(const float* __restrict__ ly_w, const float* __restrict__ ly_b, const double (&yv)[PH_MAX_NZ],
                                        int c, int nz) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < PH_MAX_NZ; ++j)
        if (j < nz) s += (double)ly_w[(size_t)c * nz + j] * yv[j];
    return s + (double)ly_b[c];
}

// the two values of row b before the sigmoid: border cells (s + psi.bias) and the centre (+ sum_c psi.weight[c] h[b][c])
__device__ __forceinline__ void ph_row_logits(const ProjRowArgs& a, int b, const double (&yv)[PH_MAX_NZ], double* scratch, double& border,
                                              double& centre) {
    const float* hr = a.h + (size_t)b * a.C;
    double s = 0.0, t = 0.0;
    for (int c = threadIdx.x; c < a.C; c += PH_THREADS) {
        const double hh = (double)hr[c];
        s += hh * ph_wy(a.ly_w, a.ly_b, yv, c, a.nz);
        t += hh * (double)a.psi_w[c];
    }
    s = block_sum_d<PH_WAVES>(s, scratch);
    t = block_sum_d<PH_WAVES>(t, scratch);
    border = s + (double)a.psi_b[0];
    centre = border + t;
}

__device__ __forceinline__ void ph_load_y(const ProjRowArgs& a, int b, double (&yv)[PH_MAX_NZ]) {
    const float* yr = a.y + (size_t)(a.By == 1 ? 0 : b) * a.nz;
#pragma unroll
    for (int j = 0; j < PH_MAX_NZ; ++j) yv[j] = j < a.nz ? (double)yr[j] : 0.0;
}

__device__ __forceinline__ double ph_sigmoid(double z) { return 1.0 / (1.0 + exp(-z)); }

// ---- forward, launch 2: one workgroup per batch row ---------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(PH_THREADS) proj_out_kernel(const ProjRowArgs a, T* __restrict__ out) {
    __shared__ double scratch[PH_WAVES];
    const int b = blockIdx.x;
    double yv[PH_MAX_NZ];
    ph_load_y(a, b, yv);
    double border, centre;
    ph_row_logits(a, b, yv, scratch, border, centre);
    if (threadIdx.x < 9) {
        double z = threadIdx.x == 4 ? centre : border;
        if (a.sigmoid) z = ph_sigmoid(z);
        st1(out + (size_t)b * 9 + threadIdx.x, (float)z);
    }
}

// ---- backward, launch 1: one workgroup per batch row ---------------------------------------------------------------------------------
// workspace (doubles): [0, B) G[b] = sum of the row's nine gradients, [B, 2 B) gc[b] = the centre's, [2 B, 2 B + B nz) the row's share of
// dy when y has batch 1 (the second launch sums them over b); with the sigmoid the gradients are first multiplied by o (1 - o) of the
// output recomputed here in float64
template <typename T>
__global__ void __launch_bounds__(PH_THREADS) proj_bwd_row_kernel(const ProjRowArgs a, const T* __restrict__ g, double* __restrict__ ws,
                                                                  float* __restrict__ dy) {
    __shared__ double scratch[PH_WAVES];
    __shared__ double Gs;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double yv[PH_MAX_NZ];
    ph_load_y(a, b, yv);
    double fb = 1.0, fc = 1.0;
    if (a.sigmoid) {
        double border, centre;
        ph_row_logits(a, b, yv, scratch, border, centre);
        const double ob = ph_sigmoid(border), oc = ph_sigmoid(centre);
        fb = ob * (1.0 - ob);
        fc = oc * (1.0 - oc);
    }
    if (tid == 0) {
        double G = 0.0, gc = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double gi = (double)ld1(g + (size_t)b * 9 + i) * (i == 4 ? fc : fb);
            G += gi;
            if (i == 4) gc = gi;
        }
        ws[b] = G;
        ws[a.B + b] = gc;
        Gs = G;
    }
    if (dy == nullptr) return;
    __syncthreads();
    const double G = Gs;
    const float* hr = a.h + (size_t)b * a.C;
    // dy[b][j] = G[b] sum_c h[b][c] l_y.weight[c][j]: one wave per j, lanes stride over c
    for (int j = wave; j < a.nz; j += PH_WAVES) {
        double s = 0.0;
        for (int c = lane; c < a.C; c += 64) s += (double)hr[c] * (double)a.ly_w[(size_t)c * a.nz + j];
        s = wave_sum_d(s) * G;
        if (lane == 0) {
            if (a.By == 1) ws[2 * (size_t)a.B + (size_t)b * a.nz + j] = s;
            else dy[(size_t)b * a.nz + j] = (float)s;
        }
    }
}

struct ProjBwdArgs {
    ProjRowArgs r;
    const double* ws;
    float *dpsi_w, *dpsi_b, *dly_w, *dly_b, *dy;
    int HW, planes, vec, accumulate, dp_blocks, c_blocks;
};

// ---- backward, launch 2 -----------------------------------------------------------------------------------------------------------------
// workgroups [0, dp_blocks): dp of PH_PLANES planes, dp[b][c][:] = G[b] wy[b][c] + gc[b] psi.weight[c];  the next c_blocks: the
// gradients that are per channel (a thread owns one c and walks b in order);  the last one: dpsi.bias and, when y has batch 1, dy.
template <typename T>
__global__ void __launch_bounds__(PH_THREADS) proj_bwd_main_kernel(const ProjBwdArgs a, T* __restrict__ dp) {
    constexpr int V = PhVec<T>::N;
    const int tid = threadIdx.x, B = a.r.B, C = a.r.C, nz = a.r.nz;
    int blk = blockIdx.x;
    if (blk < a.dp_blocks) {
        __shared__ float dh[PH_PLANES];
        const int plane0 = blk * PH_PLANES;
        const int np = min(PH_PLANES, a.planes - plane0);
        if (tid < np) {
            const int plane = plane0 + tid, b = plane / C, c = plane - b * C;
            double yv[PH_MAX_NZ];
            ph_load_y(a.r, b, yv);
            dh[tid] = (float)(a.ws[b] * ph_wy(a.r.ly_w, a.r.ly_b, yv, c, nz) + a.ws[B + b] * (double)a.r.psi_w[c]);
        }
        __syncthreads();
        const int total = np * a.HW;
        T* base = dp + (size_t)plane0 * a.HW;
        for (int o = tid * V; o < total; o += PH_THREADS * V) {
            float v[V];
            const int n = min(V, total - o);
            int q = o / a.HW, r = o - q * a.HW;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                v[i] = dh[min(q, np - 1)];
                if (++r == a.HW) { r = 0; ++q; }
            }
            if (n == V) {
                ph_store(base + o, v, a.vec);
            } else {
                for (int i = 0; i < n; ++i) st1(base + o + i, v[i]);
            }
        }
        return;
    }
    blk -= a.dp_blocks;
    if (blk < a.c_blocks) {
        const int c = blk * PH_THREADS + tid;
        if (c >= C) return;
        double sw = 0.0, sb = 0.0, sl[PH_MAX_NZ];
#pragma unroll
        for (int j = 0; j < PH_MAX_NZ; ++j) sl[j] = 0.0;
        for (int b = 0; b < B; ++b) {
            const double hh = (double)a.r.h[(size_t)b * C + c];
            const double gh = a.ws[b] * hh;
            sw += a.ws[B + b] * hh;
            sb += gh;
            if (a.dly_w) {
                const float* yr = a.r.y + (size_t)(a.r.By == 1 ? 0 : b) * nz;
#pragma unroll
                for (int j = 0; j < PH_MAX_NZ; ++j)
                    if (j < nz) sl[j] += gh * (double)yr[j];
            }
        }
        if (a.dpsi_w) a.dpsi_w[c] = (float)(a.accumulate ? sw + (double)a.dpsi_w[c] : sw);
        if (a.dly_b) a.dly_b[c] = (float)(a.accumulate ? sb + (double)a.dly_b[c] : sb);
        if (a.dly_w) {
#pragma unroll
            for (int j = 0; j < PH_MAX_NZ; ++j)
                if (j < nz) {
                    float* o = a.dly_w + (size_t)c * nz + j;
                    *o = (float)(a.accumulate ? sl[j] + (double)*o : sl[j]);
                }
        }
        return;
    }
    if (a.dpsi_b && tid == PH_MAX_NZ) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += a.ws[b];
        a.dpsi_b[0] = (float)(a.accumulate ? s + (double)a.dpsi_b[0] : s);
    }
    if (a.dy && a.r.By == 1 && tid < nz) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += a.ws[2 * (size_t)B + (size_t)b * nz + tid];
        a.dy[tid] = (float)s;
    }
}

static bool proj_sizes_ok(const char* what, int B, int C, int HW, int nz, int By, int dtype) {
    if (dtype != PCGAN_F32 && dtype != PCGAN_BF16) {
        set_error("%s: unknown dtype %d (PCGAN_F32 / PCGAN_BF16)", what, dtype);
        return false;
    }
    if (B < 1 || C < 1 || HW < 1 || HW > PH_MAX_HW || (long long)B * C > 0x7fffffffLL - PH_PLANES) {
        set_error("%s: B %d C %d HW %d outside B >= 1, C >= 1, 1 <= HW <= %d, B * C < 2^31", what, B, C, HW, PH_MAX_HW);
        return false;
    }
    if (nz < 1 || nz > PH_MAX_NZ) {
        set_error("%s: nz %d outside 1 .. %d", what, nz, PH_MAX_NZ);
        return false;
    }
    if (By != 1 && By != B) {
        set_error("%s: y has batch By %d, neither 1 nor B = %d", what, By, B);
        return false;
    }
    return true;
}

static ProjRowArgs proj_row_args(const float* h, const float* y, const float* psi_w, const float* psi_b, const float* ly_w, const float* ly_b,
                                 int B, int C, int nz, int By, int sigmoid) {
    ProjRowArgs r;
    r.h = h; r.y = y; r.psi_w = psi_w; r.psi_b = psi_b; r.ly_w = ly_w; r.ly_b = ly_b;
    r.B = B; r.C = C; r.nz = nz; r.By = By; r.sigmoid = sigmoid ? 1 : 0;
    return r;
}

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_proj_head_fwd(const void* p, const float* y, const float* psi_w, const float* psi_b, const float* ly_w,
                                   const float* ly_b, void* out, float* h, int B, int C, int HW, int nz, int By, int sigmoid, int dtype,
                                   pcgan_stream_t s) {
    if (!proj_sizes_ok("proj_head_fwd", B, C, HW, nz, By, dtype)) return 1;
    PCGAN_CHECK(p && y && psi_w && psi_b && ly_w && ly_b, "proj_head_fwd: null p / y / psi / l_y");
    PCGAN_CHECK(out && h, "proj_head_fwd: null out / h");
    const int planes = B * C;
    const int vec = (reinterpret_cast<size_t>(p) & 15) == 0 ? 1 : 0;
    const ProjRowArgs r = proj_row_args(h, y, psi_w, psi_b, ly_w, ly_b, B, C, nz, By, sigmoid);
    const unsigned blocks = (unsigned)((planes + PH_PLANES - 1) / PH_PLANES);
    PCGAN_DTYPE_SWITCH(dtype, T, {
        hipLaunchKernelGGL(proj_plane_sum_kernel<T>, dim3(blocks), dim3(PH_THREADS), 0, (hipStream_t)s, (const T*)p, h, planes, HW, vec);
        PCGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL(proj_out_kernel<T>, dim3(B), dim3(PH_THREADS), 0, (hipStream_t)s, r, (T*)out);
    });
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t pcgan_proj_head_bwd_workspace_bytes(int B, int nz) {
    return (B >= 1 && nz >= 1 && nz <= PH_MAX_NZ) ? ((size_t)2 * B + (size_t)B * nz) * sizeof(double) : 0;
}

extern "C" int pcgan_proj_head_bwd(const void* g, const float* h, const float* y, const float* psi_w, const float* psi_b,
                                   const float* ly_w, const float* ly_b, void* dp, float* dpsi_w, float* dpsi_b, float* dly_w,
                                   float* dly_b, float* dy, void* workspace, size_t workspace_bytes, int B, int C, int HW, int nz, int By,
                                   int sigmoid, int accumulate, int dtype, pcgan_stream_t s) {
    if (!proj_sizes_ok("proj_head_bwd", B, C, HW, nz, By, dtype)) return 1;
    PCGAN_CHECK(g && h && y && psi_w && psi_b && ly_w && ly_b, "proj_head_bwd: null g / h / y / psi / l_y");
    PCGAN_CHECK(dp || dpsi_w || dpsi_b || dly_w || dly_b || dy, "proj_head_bwd: nothing to compute (every output is NULL)");
    PCGAN_CHECK(workspace && workspace_bytes >= pcgan_proj_head_bwd_workspace_bytes(B, nz), "proj_head_bwd: workspace of %zu bytes, need %zu",
                workspace_bytes, pcgan_proj_head_bwd_workspace_bytes(B, nz));
    PCGAN_CHECK((reinterpret_cast<size_t>(workspace) & 7) == 0, "proj_head_bwd: the workspace must be 8-byte aligned");
    ProjBwdArgs a;
    a.r = proj_row_args(h, y, psi_w, psi_b, ly_w, ly_b, B, C, nz, By, sigmoid);
    a.ws = (const double*)workspace;
    a.dpsi_w = dpsi_w; a.dpsi_b = dpsi_b; a.dly_w = dly_w; a.dly_b = dly_b; a.dy = dy;
    a.HW = HW;
    a.planes = B * C;
    a.vec = (reinterpret_cast<size_t>(dp) & 15) == 0 ? 1 : 0;
    a.accumulate = accumulate ? 1 : 0;
    a.dp_blocks = dp ? (a.planes + PH_PLANES - 1) / PH_PLANES : 0;
    a.c_blocks = (dpsi_w || dly_w || dly_b) ? (C + PH_THREADS - 1) / PH_THREADS : 0;
    const int tail = (dpsi_b || (dy && By == 1)) ? 1 : 0;
    const unsigned blocks = (unsigned)(a.dp_blocks + a.c_blocks + tail);
    PCGAN_DTYPE_SWITCH(dtype, T, {
        hipLaunchKernelGGL(proj_bwd_row_kernel<T>, dim3(B), dim3(PH_THREADS), 0, (hipStream_t)s, a.r, (const T*)g, (double*)workspace, dy);
        PCGAN_LAUNCH_CHECK();
        if (blocks > 0) hipLaunchKernelGGL(proj_bwd_main_kernel<T>, dim3(blocks), dim3(PH_THREADS), 0, (hipStream_t)s, a, (T*)dp);
    });
    PCGAN_LAUNCH_CHECK();
    return 0;
}
