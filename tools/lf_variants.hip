// Microbenchmark: launch-geometry variants of the diag leapfrog + elementwise-gradient loop at the
// headline shape (rows of 1 024 floats), to see how far the product kernels are from what the
// memory system gives a plain flat sweep of the same bytes.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/lf_variants.hip -o tools/lf_variants
//   tools/lf_variants 1          launch-geometry table and the callable's forms (pseudo-random data)
//   tools/lf_variants 1 policy   per-array cache policy of the product-shaped loop (profiles/l2_policy)
//   tools/lf_variants 1 policy e one row of that table at 16 384 rows, three loops, for a counter run
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
struct alignas(16) F4 { float x, y, z, w; };
#define D4 256  // float4 per row (D = 1024)

__device__ __forceinline__ void lf_math(F4& pp, const F4& gg, F4& qq, const F4& mm, float h, float ed) {
  pp.x = fmaf(h, gg.x, pp.x); pp.y = fmaf(h, gg.y, pp.y); pp.z = fmaf(h, gg.z, pp.z); pp.w = fmaf(h, gg.w, pp.w);
  pp.x = fmaf(h, gg.x, pp.x); pp.y = fmaf(h, gg.y, pp.y); pp.z = fmaf(h, gg.z, pp.z); pp.w = fmaf(h, gg.w, pp.w);
  qq.x = fmaf(ed, mm.x * pp.x, qq.x); qq.y = fmaf(ed, mm.y * pp.y, qq.y);
  qq.z = fmaf(ed, mm.z * pp.z, qq.z); qq.w = fmaf(ed, mm.w * pp.w, qq.w);
}

// A: one row per wave, 4 unrolled float4 per array (the product kernel's shape); REV sweeps last-to-first
template <bool REV>
__global__ void __launch_bounds__(256) lf_row(F4* q, F4* p, const F4* __restrict__ g, const F4* __restrict__ imm,
                                              size_t N, float h, float ed) {
  const int lane = threadIdx.x & 63;
  size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  if (REV) r = N - 1 - r;
  const size_t base = r * D4;
  F4 pp[4], gg[4], qq[4], mm[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) { pp[u] = p[base + lane + 64 * u]; gg[u] = g[base + lane + 64 * u]; qq[u] = q[base + lane + 64 * u]; mm[u] = imm[lane + 64 * u]; }
#pragma unroll
  for (int u = 0; u < 4; ++u) { lf_math(pp[u], gg[u], qq[u], mm[u], h, ed); p[base + lane + 64 * u] = pp[u]; q[base + lane + 64 * u] = qq[u]; }
}

// B: flat grid-stride over float4 elements, U independent elements in flight per thread
template <int U>
__global__ void __launch_bounds__(256) lf_flat(F4* q, F4* p, const F4* __restrict__ g, const F4* __restrict__ imm,
                                               size_t n4, float h, float ed) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += stride * U) {
    F4 pp[U], gg[U], qq[U], mm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const size_t i = i0 + u * stride; if (i < n4) { pp[u] = p[i]; gg[u] = g[i]; qq[u] = q[i]; mm[u] = imm[i & (D4 - 1)]; } }
#pragma unroll
    for (int u = 0; u < U; ++u) { const size_t i = i0 + u * stride; if (i < n4) { lf_math(pp[u], gg[u], qq[u], mm[u], h, ed); p[i] = pp[u]; q[i] = qq[u]; } }
  }
}

// C: a block of 256 threads owns 4 consecutive rows as one 16 KB span; thread t takes float4 t, t+256, ...
__global__ void __launch_bounds__(256) lf_span(F4* q, F4* p, const F4* __restrict__ g, const F4* __restrict__ imm,
                                               size_t n4, float h, float ed) {
  const size_t base = (size_t)blockIdx.x * 1024;
  F4 pp[4], gg[4], qq[4], mm[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) { const size_t i = base + threadIdx.x + 256 * u; if (i < n4) { pp[u] = p[i]; gg[u] = g[i]; qq[u] = q[i]; mm[u] = imm[i & (D4 - 1)]; } }
#pragma unroll
  for (int u = 0; u < 4; ++u) { const size_t i = base + threadIdx.x + 256 * u; if (i < n4) { lf_math(pp[u], gg[u], qq[u], mm[u], h, ed); p[i] = pp[u]; q[i] = qq[u]; } }
}

// gradient of a diagonal Gaussian: g = -(q - mu) * prec (elementwise), one row per wave / flat
__global__ void __launch_bounds__(256) grad_row(const F4* __restrict__ q, F4* __restrict__ g, const F4* __restrict__ mu,
                                                const F4* __restrict__ pr, size_t N) {
  const int lane = threadIdx.x & 63;
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const size_t base = r * D4;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const F4 a = q[base + lane + 64 * u], m = mu[lane + 64 * u], s = pr[lane + 64 * u];
    g[base + lane + 64 * u] = F4{-(a.x - m.x) * s.x, -(a.y - m.y) * s.y, -(a.z - m.z) * s.z, -(a.w - m.w) * s.w};
  }
}
template <int U>
__global__ void __launch_bounds__(256) grad_flat(const F4* __restrict__ q, F4* __restrict__ g, const F4* __restrict__ mu,
                                                 const F4* __restrict__ pr, size_t n4) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += stride * U) {
    F4 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const size_t i = i0 + u * stride; if (i < n4) a[u] = q[i]; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * stride;
      if (i < n4) { const F4 m = mu[i & (D4 - 1)], s = pr[i & (D4 - 1)];
        g[i] = F4{-(a[u].x - m.x) * s.x, -(a[u].y - m.y) * s.y, -(a[u].z - m.z) * s.z, -(a[u].w - m.w) * s.w}; }
    }
  }
}

// ---- the callable of the headline bench (DiagGaussian: g = -(q*inv_var), logp = 0.5 sum q*g) in its two forms,
// run in the product's order: leapfrog (one piece per lane, last row first) ; callable (first row first)
__global__ void __launch_bounds__(256) lf_piece_rev(F4* q, F4* p, const F4* __restrict__ g, const F4* __restrict__ imm,
                                                    float h, float ed) {
  const size_t i = (size_t)(gridDim.x - 1 - blockIdx.x) * 256 + threadIdx.x;
  F4 pp = p[i], gg = g[i], qq = q[i];
  const F4 mm = imm[threadIdx.x];
  lf_math(pp, gg, qq, mm, h, ed);
  p[i] = pp; q[i] = qq;
}
// row + reduction (k_diag_gaussian<4>): one wave per row, fp64 sum of q*g, wave reduction, logp store
__global__ void __launch_bounds__(256) call_row_logp(const F4* __restrict__ q, F4* __restrict__ g, const F4* __restrict__ iv,
                                                     float* __restrict__ logp, size_t N) {
  const int lane = threadIdx.x & 63;
  for (size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < N; r += (size_t)gridDim.x * 4) {
    const size_t base = r * D4;
    F4 a[4], v[4];
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { a[u] = q[base + lane + 64 * u]; v[u] = iv[lane + 64 * u]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const F4 o{-(a[u].x * v[u].x), -(a[u].y * v[u].y), -(a[u].z * v[u].z), -(a[u].w * v[u].w)};
      acc += (double)a[u].x * (double)o.x; acc += (double)a[u].y * (double)o.y;
      acc += (double)a[u].z * (double)o.z; acc += (double)a[u].w * (double)o.w;
      g[base + lane + 64 * u] = o;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) logp[r] = (float)(0.5 * acc);
  }
}
// flat gradient-only (k_diag_gaussian_grad_flat<.>): one piece per lane, one workgroup per 4 KB span, ascending;
// XCD = true is the product's numbering (grad_span_of_workgroup)
// XCD: workgroup b runs on XCD b % 8 and lf_piece_rev gives span s to workgroup grid - 1 - s, i.e. (grid % 8 == 0) to
// XCD 7 - s % 8; with b ^ 7 the callable reads and writes span s on that same XCD (its 4 MiB L2 is not shared)
template <bool XCD>
__global__ void __launch_bounds__(256) call_piece_grad(const F4* __restrict__ q, F4* __restrict__ g,
                                                       const F4* __restrict__ iv) {
  const size_t i = (size_t)(XCD ? blockIdx.x ^ 7u : blockIdx.x) * 256 + threadIdx.x;
  const F4 a = q[i], v = iv[threadIdx.x];
  g[i] = F4{-(a.x * v.x), -(a.y * v.y), -(a.z * v.z), -(a.w * v.w)};
}

// ---- per-array cache policy of the product-shaped loop (lf_piece_rev ; call_piece_grad<true>): each of the three
// stored arrays (p, q in the leapfrog, g in the callable) takes a store flavour, the leapfrog's load of p a load flavour.
// PLAIN and NTP keep the line in the XCD's L2; SC1 writes through and drops it (buffer store with aux = 16; the
// descriptor covers the workgroup's own 4 KB span, so it is built from workgroup-uniform values only).
enum { PLAIN = 0, NTP = 1, SC1 = 2 };
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
template <int POL> __device__ __forceinline__ void st_pol(F4* span, F4 v) {
  if constexpr (POL == SC1) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(span, 0, 4096, 0x00020000);
    const u4v t = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, (int)(threadIdx.x * 16), 0, 16);
  } else if constexpr (POL == NTP) {
    const f4v t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f4v*>(span + threadIdx.x));
  } else {
    span[threadIdx.x] = v;
  }
}
template <int SP, int SQ, int LP>
__global__ void __launch_bounds__(256) lf_piece_rev_pol(F4* q, F4* p, const F4* __restrict__ g,
                                                        const F4* __restrict__ imm, float h, float ed) {
  const size_t s = (size_t)(gridDim.x - 1 - blockIdx.x) * 256, i = s + threadIdx.x;
  F4 pp;
  if constexpr (LP == NTP) { const f4v t = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p + i)); pp = F4{t.x, t.y, t.z, t.w}; }
  else pp = p[i];
  F4 gg = g[i], qq = q[i];
  const F4 mm = imm[threadIdx.x];
  lf_math(pp, gg, qq, mm, h, ed);
  st_pol<SP>(p + s, pp); st_pol<SQ>(q + s, qq);
}
template <int SG>
__global__ void __launch_bounds__(256) call_piece_grad_pol(const F4* __restrict__ q, F4* __restrict__ g,
                                                           const F4* __restrict__ iv) {
  const size_t s = (size_t)(blockIdx.x ^ 7u) * 256;
  const F4 a = q[s + threadIdx.x], v = iv[threadIdx.x];
  st_pol<SG>(g + s, F4{-(a.x * v.x), -(a.y * v.y), -(a.z * v.z), -(a.w * v.w)});
}
// order-independent sum of the bit patterns: every policy must leave the bits the plain stores leave
__global__ void bits_sum(const unsigned* a, size_t n, unsigned long long* out) {
  unsigned long long s = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    s += (unsigned long long)a[i] * (unsigned long long)((i & 1023) + 1);
  atomicAdd(out, s);
}

// pseudo-random fill: all-zero buffers toggle no data lines and flatter a power-limited part
__global__ void fill_random(float* a, size_t n, unsigned seed, float lo, float hi) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    a[i] = lo + (hi - lo) * (float)(x >> 8) * (1.0f / 16777216.0f);
  }
}

typedef void (*lf_fn)(F4*, F4*, const F4*, const F4*, float, float);
typedef void (*gr_fn)(const F4*, F4*, const F4*);
static const char* kPolName[3] = {"plain", "nt", "sc1"};
static double median_of(const float* v, int n) {
  float t[16]; std::copy(v, v + n, t); std::sort(t, t + n); return t[n / 2];
}

// per-array policy table: rows interleaved inside each of five repeats, one process
static int policy_main(const char* only) {
  const int L = 50, REPS = 5, LOOPS = 6;
  struct Desc { const char* name; int sp, sq, sg, lp; lf_fn lf; gr_fn gr; };
  const Desc rows[] = {
      {"parent", PLAIN, PLAIN, PLAIN, PLAIN, lf_piece_rev_pol<PLAIN, PLAIN, PLAIN>, call_piece_grad_pol<PLAIN>},
      {"a", SC1, PLAIN, PLAIN, PLAIN, lf_piece_rev_pol<SC1, PLAIN, PLAIN>, call_piece_grad_pol<PLAIN>},
      {"b", SC1, PLAIN, PLAIN, NTP, lf_piece_rev_pol<SC1, PLAIN, NTP>, call_piece_grad_pol<PLAIN>},
      {"c", SC1, NTP, PLAIN, PLAIN, lf_piece_rev_pol<SC1, NTP, PLAIN>, call_piece_grad_pol<PLAIN>},
      {"d", SC1, SC1, PLAIN, PLAIN, lf_piece_rev_pol<SC1, SC1, PLAIN>, call_piece_grad_pol<PLAIN>},
      {"e", SC1, PLAIN, SC1, PLAIN, lf_piece_rev_pol<SC1, PLAIN, PLAIN>, call_piece_grad_pol<SC1>},
      {"f", SC1, SC1, SC1, PLAIN, lf_piece_rev_pol<SC1, SC1, PLAIN>, call_piece_grad_pol<SC1>},
      {"g", SC1, NTP, NTP, PLAIN, lf_piece_rev_pol<SC1, NTP, PLAIN>, call_piece_grad_pol<NTP>},
      {"h", NTP, PLAIN, PLAIN, PLAIN, lf_piece_rev_pol<NTP, PLAIN, PLAIN>, call_piece_grad_pol<PLAIN>},
      {"i", NTP, PLAIN, PLAIN, NTP, lf_piece_rev_pol<NTP, PLAIN, NTP>, call_piece_grad_pol<PLAIN>},
  };
  const int R = (int)(sizeof(rows) / sizeof(rows[0]));
  F4 *q, *p, *g, *imm, *iv;
  unsigned long long* sum;
  const size_t maxN = 65536;
  hipMalloc(&q, maxN * D4 * 16); hipMalloc(&p, maxN * D4 * 16); hipMalloc(&g, maxN * D4 * 16);
  hipMalloc(&imm, D4 * 16); hipMalloc(&iv, D4 * 16); hipMalloc(&sum, 3 * 8);
  fill_random<<<4, 256>>>((float*)imm, 1024, 4u, 0.5f, 2.0f);
  fill_random<<<4, 256>>>((float*)iv, 1024, 6u, 0.5f, 2.0f);
  hipEvent_t e0, e1, e2; hipEventCreate(&e0); hipEventCreate(&e1); hipEventCreate(&e2);
  const float h = 0.125f, ed = 0.25f;  // eps^2 * imm * inv_var <= 0.25: the loop's orbit stays bounded
  auto refill = [&](size_t N) {
    fill_random<<<4096, 256>>>((float*)q, N * 1024, 1u, -1.0f, 1.0f);
    fill_random<<<4096, 256>>>((float*)p, N * 1024, 2u, -1.0f, 1.0f);
    fill_random<<<4096, 256>>>((float*)g, N * 1024, 3u, -1.0f, 1.0f);
  };
  if (only) {
    const size_t N = 16384;
    const unsigned pieces = (unsigned)(N * D4 / 256);
    for (int r = 0; r < R; ++r) {
      if (strcmp(rows[r].name, only)) continue;
      refill(N);
      for (int s = 0; s < 3 * L; ++s) { rows[r].lf<<<pieces, 256>>>(q, p, g, imm, h, ed); rows[r].gr<<<pieces, 256>>>(q, g, iv); }
      hipDeviceSynchronize();
      printf("row %s: %d steps at %zu rows\n", only, 3 * L, N);
      return 0;
    }
    fprintf(stderr, "no such row: %s\n", only);
    return 2;
  }
  printf("data: pseudo-random; loop = lf_piece_rev ; call_piece_grad<XCD>, %d steps per loop, %d timed loops per repeat, "
         "%d repeats (rows interleaved inside each repeat)\n", L, LOOPS, REPS);
  int bad = 0;
  for (size_t N : {(size_t)16384, (size_t)65536}) {
    const unsigned pieces = (unsigned)(N * D4 / 256);
    // every policy leaves the parent's bits (one loop from the same start)
    unsigned long long ref[3] = {0, 0, 0};
    for (int r = 0; r < R; ++r) {
      refill(N);
      for (int s = 0; s < L; ++s) { rows[r].lf<<<pieces, 256>>>(q, p, g, imm, h, ed); rows[r].gr<<<pieces, 256>>>(q, g, iv); }
      hipMemset(sum, 0, 24);
      bits_sum<<<2048, 256>>>((const unsigned*)q, N * 1024, sum);
      bits_sum<<<2048, 256>>>((const unsigned*)p, N * 1024, sum + 1);
      bits_sum<<<2048, 256>>>((const unsigned*)g, N * 1024, sum + 2);
      unsigned long long hs[3];
      hipMemcpy(hs, sum, 24, hipMemcpyDeviceToHost);
      if (r == 0) std::copy(hs, hs + 3, ref);
      const bool same = hs[0] == ref[0] && hs[1] == ref[1] && hs[2] == ref[2];
      if (!same) { ++bad; printf("N %6zu row %-6s : BITS DIFFER from parent\n", N, rows[r].name); }
    }
    printf("N %6zu : q, p, g after one loop %s\n", N, bad ? "DIFFER" : "bit-identical to the parent in every row");
    static float loop[16][REPS], lfa[16][REPS], gra[16][REPS];
    for (int rep = 0; rep < REPS; ++rep) {
      for (int r = 0; r < R; ++r) {
        auto lf = [&]() { rows[r].lf<<<pieces, 256>>>(q, p, g, imm, h, ed); };
        auto gr = [&]() { rows[r].gr<<<pieces, 256>>>(q, g, iv); };
        refill(N);
        for (int s = 0; s < L; ++s) { lf(); gr(); }  // warm, untimed
        refill(N);
        hipEventRecord(e0);
        for (int s = 0; s < LOOPS * L; ++s) { lf(); gr(); }
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        loop[r][rep] = ms * 1e3f / (LOOPS * L);
        refill(N);
        hipEventRecord(e0);
        for (int s = 0; s < LOOPS * L; ++s) lf();
        hipEventRecord(e1);
        for (int s = 0; s < LOOPS * L; ++s) gr();
        hipEventRecord(e2);
        hipEventSynchronize(e2);
        float a, b; hipEventElapsedTime(&a, e0, e1); hipEventElapsedTime(&b, e1, e2);
        lfa[r][rep] = a * 1e3f / (LOOPS * L); gra[r][rep] = b * 1e3f / (LOOPS * L);
      }
    }
    const double pmed = median_of(loop[0], REPS);
    const double pspread = *std::max_element(loop[0], loop[0] + REPS) - *std::min_element(loop[0], loop[0] + REPS);
    printf("N %6zu : parent loop median %.2f us/step, max - min %.2f ; candidate threshold: median < %.2f\n", N, pmed, pspread,
           pmed - 3.0 * pspread);
    for (int r = 0; r < R; ++r) {
      const double med = median_of(loop[r], REPS);
      printf("N %6zu row %-6s p-st %-5s q-st %-5s g-st %-5s p-ld %-5s | loop us/step", N, rows[r].name, kPolName[rows[r].sp],
             kPolName[rows[r].sq], kPolName[rows[r].sg], kPolName[rows[r].lp]);
      for (int k = 0; k < REPS; ++k) printf(" %6.2f", loop[r][k]);
      printf(" median %6.2f | lf alone", med);
      for (int k = 0; k < REPS; ++k) printf(" %6.2f", lfa[r][k]);
      printf(" median %6.2f | grad alone", median_of(lfa[r], REPS));
      for (int k = 0; k < REPS; ++k) printf(" %6.2f", gra[r][k]);
      printf(" median %6.2f | %s\n", median_of(gra[r], REPS),
             r == 0 ? "parent" : med < pmed - 3.0 * pspread ? "CANDIDATE" : "no candidate");
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  const int L = 50;
  const bool randomize = argc > 1 && atoi(argv[1]) != 0;
  if (argc > 2 && !strcmp(argv[2], "policy")) return policy_main(argc > 3 ? argv[3] : nullptr);
  F4 *q, *p, *g, *imm, *mu, *pr;
  const size_t maxN = 65536;
  hipMalloc(&q, maxN * D4 * 16); hipMalloc(&p, maxN * D4 * 16); hipMalloc(&g, maxN * D4 * 16);
  hipMalloc(&imm, D4 * 16); hipMalloc(&mu, D4 * 16); hipMalloc(&pr, D4 * 16);
  hipMemset(q, 0, maxN * D4 * 16); hipMemset(p, 0, maxN * D4 * 16); hipMemset(g, 0, maxN * D4 * 16);
  hipMemset(imm, 0, D4 * 16); hipMemset(mu, 0, D4 * 16); hipMemset(pr, 0, D4 * 16);
  if (randomize) {
    fill_random<<<4096, 256>>>((float*)q, maxN * 1024, 1u, -1.0f, 1.0f);
    fill_random<<<4096, 256>>>((float*)p, maxN * 1024, 2u, -1.0f, 1.0f);
    fill_random<<<4096, 256>>>((float*)g, maxN * 1024, 3u, -1.0f, 1.0f);
    fill_random<<<4, 256>>>((float*)imm, 1024, 4u, 0.5f, 2.0f);
    fill_random<<<4, 256>>>((float*)mu, 1024, 5u, -1.0f, 1.0f);
    fill_random<<<4, 256>>>((float*)pr, 1024, 6u, 0.5f, 2.0f);
  }
  printf("data: %s\n", randomize ? "pseudo-random" : "zeros");
  hipEvent_t e0, e1, e2; hipEventCreate(&e0); hipEventCreate(&e1); hipEventCreate(&e2);
  const float h = 0.125f, ed = 0.25f;
  for (size_t N : {(size_t)16384, (size_t)65536}) {
    const size_t n4 = N * D4;
    const unsigned rowgrid = (unsigned)(N / 4);
    for (int v = 0; v < 9; ++v) {
      auto lf = [&]() {
        switch (v) {
          case 0: lf_row<false><<<rowgrid, 256>>>(q, p, g, imm, N, h, ed); break;
          case 1: lf_row<true><<<rowgrid, 256>>>(q, p, g, imm, N, h, ed); break;
          case 2: lf_flat<4><<<(unsigned)(n4 / 1024), 256>>>(q, p, g, imm, n4, h, ed); break;
          case 3: lf_flat<4><<<2048, 256>>>(q, p, g, imm, n4, h, ed); break;
          case 4: lf_flat<2><<<4096, 256>>>(q, p, g, imm, n4, h, ed); break;
          case 5: lf_flat<1><<<4096, 256>>>(q, p, g, imm, n4, h, ed); break;
          case 6: lf_flat<1><<<(unsigned)(n4 / 256), 256>>>(q, p, g, imm, n4, h, ed); break;
          case 7: lf_span<<<(unsigned)(n4 / 1024), 256>>>(q, p, g, imm, n4, h, ed); break;
          case 8: lf_flat<8><<<1024, 256>>>(q, p, g, imm, n4, h, ed); break;
        }
      };
      auto gr = [&]() {
        if (v == 0 || v == 1 || v == 7) grad_row<<<rowgrid, 256>>>(q, g, mu, pr, N);
        else if (v == 6) grad_flat<1><<<(unsigned)(n4 / 256), 256>>>(q, g, mu, pr, n4);
        else grad_flat<4><<<(unsigned)(n4 / 1024), 256>>>(q, g, mu, pr, n4);
      };
      float best_loop = 1e30f, best_lf = 1e30f, best_gr = 1e30f;
      for (int rep = 0; rep < 4; ++rep) {
        hipEventRecord(e0);
        for (int s = 0; s < L; ++s) { lf(); gr(); }
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (rep && ms < best_loop) best_loop = ms;
        // the kernels alone, back to back (same working set)
        hipEventRecord(e0);
        for (int s = 0; s < L; ++s) lf();
        hipEventRecord(e1);
        for (int s = 0; s < L; ++s) gr();
        hipEventRecord(e2);
        hipEventSynchronize(e2);
        float a, b; hipEventElapsedTime(&a, e0, e1); hipEventElapsedTime(&b, e1, e2);
        if (rep && a < best_lf) best_lf = a;
        if (rep && b < best_gr) best_gr = b;
      }
      const double bytes_lf = 20.0 * N * 1024, bytes_gr = 8.0 * N * 1024;
      printf("N %6zu v%d : loop %7.1f us/step (%5.2f TB/s of 28 B) | lf alone %6.1f us (%5.2f TB/s) | grad alone %6.1f us (%5.2f TB/s)\n",
             N, v, best_loop * 1e3 / L, (bytes_lf + bytes_gr) / (best_loop * 1e-3 / L) / 1e12, best_lf * 1e3 / L,
             bytes_lf / (best_lf * 1e-3 / L) / 1e12, best_gr * 1e3 / L, bytes_gr / (best_gr * 1e-3 / L) / 1e12);
    }
  }
  // the callable's two forms between product-shaped leapfrogs (what one HMC trajectory launches)
  float* logp; hipMalloc(&logp, maxN * 4);
  for (size_t N : {(size_t)16384, (size_t)65536}) {
    const unsigned pieces = (unsigned)(N * D4 / 256), rowgrid = (unsigned)(N / 4 < 65536 ? N / 4 : 65536);
    for (int v = 0; v < 3; ++v) {
      auto lf = [&]() { lf_piece_rev<<<pieces, 256>>>(q, p, g, imm, h, ed); };
      auto cl = [&]() {
        if (v == 0) call_row_logp<<<rowgrid, 256>>>(q, g, pr, logp, N);
        else if (v == 1) call_piece_grad<false><<<pieces, 256>>>(q, g, pr);
        else call_piece_grad<true><<<pieces, 256>>>(q, g, pr);
      };
      float best_loop = 1e30f, best_cl = 1e30f;
      for (int rep = 0; rep < 6; ++rep) {
        // q drifts under 50 leapfrogs: start every repetition from the same bounded pseudo-random state
        if (randomize) {
          fill_random<<<4096, 256>>>((float*)q, N * 1024, 1u, -1.0f, 1.0f);
          fill_random<<<4096, 256>>>((float*)p, N * 1024, 2u, -1.0f, 1.0f);
        }
        hipEventRecord(e0);
        for (int s = 0; s < L; ++s) { lf(); cl(); }
        hipEventRecord(e1);
        for (int s = 0; s < L; ++s) cl();
        hipEventRecord(e2);
        hipEventSynchronize(e2);
        float a, b; hipEventElapsedTime(&a, e0, e1); hipEventElapsedTime(&b, e1, e2);
        if (rep && a < best_loop) best_loop = a;
        if (rep && b < best_cl) best_cl = b;
      }
      const double bytes_cl = 8.0 * N * 1024;
      printf("N %6zu callable %-25s : lf+callable %7.1f us/step | callable alone %6.1f us (%5.2f TB/s of 8 B)\n", N,
             v == 0 ? "row+logp (full)" : v == 1 ? "piece-per-lane (grad)" : "piece-per-lane, same XCD", best_loop * 1e3 / L, best_cl * 1e3 / L,
             bytes_cl / (best_cl * 1e-3 / L) / 1e12);
    }
  }
  return 0;
}
