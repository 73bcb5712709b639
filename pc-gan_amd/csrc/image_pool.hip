// History of generated images: the per-image loop of the reference's ImagePool.query (util/image_pool.py:12-32) in ONE launch per
// PCGAN_POOL_PLAN_MAX images.  The random decisions are made on the host and arrive as a plan, one int32 per image, processed IN ORDER:
//     plan[i] <  0           pass      y[i] = x[i]
//     plan[i] == 2 * s       store     pool[s] = x[i]; y[i] = x[i]                (the fill phase)
//     plan[i] == 2 * s + 1   exchange  y[i] = old pool[s]; pool[s] = x[i]
// Later images see the writes of earlier ones: two images of one batch may name the same slot, and the second then receives the first.
//
// Race-free by construction: a thread owns one 16-byte vector (or one element) INDEX WITHIN THE IMAGE and walks all images of the plan
// serially for that index.  Every read and write of a given pool address therefore comes from one thread, in program order; different
// threads touch disjoint addresses of x, y and pool (the host refuses overlapping ranges).  No atomics, no LDS, no second launch, no
// workspace, and nothing is parallelised over images or slots.
//
// The plan travels inside the by-value kernel argument (PoolPlan), as AddNSrcs does in grad_fanin.hip: no device table, no upload.  Its
// entries are uniform over the grid, so the branch on them does not diverge.  A longer batch is served by consecutive launches on the
// same stream; the pool carries the state from one to the next.
//
// Pure copies, bit-exact for every payload (-0.0, NaN bits): the data is moved as unsigned words of the element width (4 bytes for
// PCGAN_F32, 2 for PCGAN_BF16) or as 16-byte vectors.  16-byte accesses need x, y, pool AND the image stride in bytes to be multiples of
// 16, since every image and slot base must be aligned; images are contiguous (stride = n elements), so where the 16-byte form applies
// it covers the whole image and its element tail is empty.  Everything else takes the element form.
//
// Bound: bytes moved, between 2 (pass) and 3 (exchange) * n_img * n * sizeof(T), but NOT at HBM rate: the parallelism is n / V threads,
// each with n_img dependent-in-order steps.  An image of 3 * 128^2 fp32 elements gives 12 288 vector threads, fewer than the machine
// has lanes, so the launch is latency-bound.  That is the price of the serial-per-index rule and is accepted: the pool moves a few
// megabytes per training step, and what the kernel saves is launches and host round trips.  Measured on one MI355X (scripts/bench_disc.py,
// profiles/disc_step.json) at [10, 3, 128, 128] fp32 against a pool of 50, every other image exchanged, from memory: 8.9 us per launch
// (0.56 TB/s) against 52 us for the reference's unsqueeze / clone / cat loop as torch ops.
#include "common.h"

namespace pcgan {

static constexpr unsigned POOL_THREADS = 256;
static constexpr unsigned POOL_MAX_BLOCKS = 2048;     // 8 workgroups per CU on 256 CUs; larger images wrap the grid-stride loop

struct PoolPlan {
    int n_img;
    int op[PCGAN_POOL_PLAN_MAX];
};

// U: the unit a thread moves (uint4, unsigned or unsigned short); nu: units per image and per pool slot
template <typename U>
__global__ void __launch_bounds__(POOL_THREADS) pool_exchange_kernel(const PoolPlan plan, const U* __restrict__ x, U* __restrict__ y, U* pool,
                                                                     const size_t nu) {
    const size_t stride = (size_t)gridDim.x * POOL_THREADS;
    for (size_t i = (size_t)blockIdx.x * POOL_THREADS + threadIdx.x; i < nu; i += stride) {
        for (int k = 0; k < plan.n_img; ++k) {          // serial over the images: this thread alone touches index i of every slot
            const int op = plan.op[k];
            U v = x[(size_t)k * nu + i];
            if (op >= 0) {
                U* slot = pool + (size_t)(op >> 1) * nu + i;
                const U in = v;
                if (op & 1) v = *slot;
                *slot = in;
            }
            y[(size_t)k * nu + i] = v;
        }
    }
}

template <typename U>
static void pool_exchange_launch(const PoolPlan& plan, const void* x, void* y, void* pool, size_t nu, hipStream_t st) {
    const dim3 grid(capped_blocks(nu, POOL_THREADS, POOL_MAX_BLOCKS)), block(POOL_THREADS);
    hipLaunchKernelGGL(pool_exchange_kernel<U>, grid, block, 0, st, plan, static_cast<const U*>(x), static_cast<U*>(y), static_cast<U*>(pool), nu);
}

static unsigned long long g_pool_launches = 0;

static inline bool pool_disjoint(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a + na <= b || b + nb <= a; }

}  // namespace pcgan

using namespace pcgan;

extern "C" unsigned long long pcgan_pool_exchange_launches(void) { return g_pool_launches; }

extern "C" int pcgan_pool_exchange(void* pool, int pool_size, const void* x, void* y, const int* plan, int n_img, size_t n, int dtype,
                                   pcgan_stream_t s) {
    PCGAN_CHECK(pool && x && y && plan, "pool_exchange: null pointer (%s)", !pool ? "pool" : (!x ? "x" : (!y ? "y" : "plan")));
    PCGAN_CHECK(n > 0, "pool_exchange: n == 0");
    PCGAN_CHECK(n_img >= 1, "pool_exchange: n_img = %d, need at least 1", n_img);
    PCGAN_CHECK(pool_size >= 1, "pool_exchange: pool_size = %d, need at least 1", pool_size);
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "pool_exchange: unknown dtype %d", dtype);
    for (int i = 0; i < n_img; ++i)
        PCGAN_CHECK(plan[i] < 0 || (plan[i] >> 1) < pool_size, "pool_exchange: image %d names slot %d outside [0, %d)", i, plan[i] >> 1,
                    pool_size);
    const size_t es = dtype == PCGAN_F32 ? 4 : 2, img_bytes = n * es;
    const size_t batch_bytes = (size_t)n_img * img_bytes, pool_bytes = (size_t)pool_size * img_bytes;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y), p0 = reinterpret_cast<uintptr_t>(pool);
    PCGAN_CHECK(pool_disjoint(x0, batch_bytes, y0, batch_bytes), "pool_exchange: x and y overlap");
    PCGAN_CHECK(pool_disjoint(x0, batch_bytes, p0, pool_bytes), "pool_exchange: x and pool overlap");
    PCGAN_CHECK(pool_disjoint(y0, batch_bytes, p0, pool_bytes), "pool_exchange: y and pool overlap");
    const bool wide = ((x0 | y0 | p0 | img_bytes) & 15u) == 0;
    hipStream_t st = (hipStream_t)s;
    for (int first = 0; first < n_img; first += PCGAN_POOL_PLAN_MAX) {      // consecutive launches: the pool carries the state
        PoolPlan a;
        a.n_img = n_img - first < PCGAN_POOL_PLAN_MAX ? n_img - first : PCGAN_POOL_PLAN_MAX;
        for (int k = 0; k < PCGAN_POOL_PLAN_MAX; ++k) a.op[k] = k < a.n_img ? plan[first + k] : -1;
        const char* xs = static_cast<const char*>(x) + (size_t)first * img_bytes;
        char* ys = static_cast<char*>(y) + (size_t)first * img_bytes;
        if (wide) pool_exchange_launch<uint4>(a, xs, ys, pool, img_bytes / 16, st);
        else if (dtype == PCGAN_F32) pool_exchange_launch<unsigned>(a, xs, ys, pool, n, st);
        else pool_exchange_launch<unsigned short>(a, xs, ys, pool, n, st);
        PCGAN_LAUNCH_CHECK();
        ++g_pool_launches;
    }
    return 0;
}
