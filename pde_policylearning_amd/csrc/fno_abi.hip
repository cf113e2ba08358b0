// fnoengine C-ABI implementation: plans (twiddle tables), workspace carving and the
// kernel sequences for the standalone spectral convolution and the fused FNO model.
// Host-side only orchestration; every kernel is hand-written HIP for gfx950.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fnoengine.h"
#include "fno_debug.h"
#include "k_block_bwd.h"
#include "k_block_bwd2.h"
#include "k_chanflow.h"
#include "k_chanflow_step.h"
#include "k_control_loop.h"
#include "k_action_opt.h"
#include "k_policy_opt.h"
#include "k_ns2d.h"
#include "k_pointwise.h"
#include "k_block_fwd2.h"
#include "k_block_fwd3.h"
#include "k_projection.h"
#include "k_projection2.h"
#include "k_projection_h2.h"
#include "k_channel_mlp.h"
#include "k_domain_pad.h"
#include "k_data_gather.h"
#include "k_pino_batch.h"
#include "k_spectral_mid.h"
#include "k_spec1d.h"
#include "k_pino_loss.h"
#include "k_pino_loss2.h"
#include "k_burgers_loss.h"
#include "k_darcy_loss.h"
#include "k_sobolev_loss.h"
#include "k_hs_loss.h"
#include "k_rno_gates.h"
#include "k_train.h"

// --------------------------------------------------------------------------
// errors
// --------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(FNO_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" int fno_version(void) { return FNO_VERSION; }

// GEMM arithmetic of the fused model path: 1 = 3-term bf16 split on the matrix cores (fp32-grade,
// default), 0 = fp32 MFMA.  FNO_GEMM_F32=1 in the environment selects 0 at load time.
static int g_gemm_x3 = []() { const char* e = getenv("FNO_GEMM_F32"); return (e && e[0] == '1') ? 0 : 1; }();
// In the split mode, two-term fp16 channel GEMMs (fno_dev.h "h2": half the matrix-pipe work of the three-term bf16 split) run
// wherever a kernel has the variant and its operands' magnitude bounds are known; the three-term kernels are what runs when
// no bound is known.
extern "C" void fno_set_gemm_mode(int x3) { g_gemm_x3 = x3 ? 1 : 0; }
extern "C" int fno_get_gemm_mode(void) { return g_gemm_x3; }
extern "C" const char* fno_last_error(void) { return g_err.c_str(); }
// mode contraction on the fp32 matrix cores (default) or the VALU kernels (FNO_MODE_GEMM_VALU=1 / fno_set_mode_gemm(0)):
// an A/B switch for profiling and for the parity tests, which run both
static int g_mode_mfma = []() { const char* e = getenv("FNO_MODE_GEMM_VALU"); return (e && e[0] == '1') ? 0 : 1; }();
extern "C" void fno_set_mode_gemm(int mfma) { g_mode_mfma = mfma ? 1 : 0; }
extern "C" int fno_get_mode_gemm(void) { return g_mode_mfma; }

// --------------------------------------------------------------------------
// optional per-kernel timing (HIP events on the launch stream)
// --------------------------------------------------------------------------
struct ProfRec { std::string name; hipEvent_t a, b; int terms; };
static bool g_prof = false;
static std::vector<ProfRec> g_recs;
struct ProfAgg { std::string name; float ms; int n; int terms; };
// which matrix pipe the NEXT launch's channel GEMMs use (read and cleared by launch(); the profile reports it so that bench.py
// prices a kernel against the peak of the pipe it ran on): 0 not stated, 1 fp32 MFMA, 2 two fp16 terms (3 products per k
// block), 3 three bf16 terms (6 products)
static thread_local int g_terms_next = 0;
#define GT(n) (g_terms_next = (n))
static std::vector<ProfAgg> g_agg;

// --------------------------------------------------------------------------
// optional launch log (tests): which kernel INSTANTIATION a dispatch site launched and with what tiling.  The profile labels
// above cannot tell ("k_rowidft_chan" names three kernels, "k_mode_gemm" five) and stay as they are: bench.py prices kernels
// by them.  A dispatch site states its variant in the launching statement itself - LV(tag, rb, ntiles), launch(...) - and
// launch() reads and clears it like g_terms_next.  Off by default: nothing is recorded and the vector holds no storage.
// Not part of include/fnoengine.h: the fno_debug_* entry points are declared in fno_debug.h.
// --------------------------------------------------------------------------
struct LaunchTag { const char* variant; int rb, ntiles; };      // rb: rows (contractions: batch rows / input channels) per workgroup; 0 = the site has none
struct LaunchRec { const char* name; LaunchTag tag; unsigned grid[3], block[3]; size_t lds; };
static thread_local LaunchTag g_tag_next = {nullptr, 0, 0};
#define LV(variant, rb, ntiles) (g_tag_next = LaunchTag{(variant), (int)(rb), (int)(ntiles)})
static bool g_llog = false;
static std::mutex g_llog_mu;
static std::vector<LaunchRec> g_llog_recs;
extern "C" void fno_debug_launch_log(int on) {      // on: start an empty log; off: stop and release it
  std::lock_guard<std::mutex> lk(g_llog_mu);
  g_llog = on != 0;
  std::vector<LaunchRec>().swap(g_llog_recs);
}
extern "C" int fno_debug_launch_count(void) {
  std::lock_guard<std::mutex> lk(g_llog_mu);
  return (int)g_llog_recs.size();
}
// name: the profile label; variant: the site's tag ("" where the site states none); grid / block: three extents each
extern "C" int fno_debug_launch_get(int i, const char** name, const char** variant, int* rb, int* ntiles, unsigned* grid,
                                    unsigned* block, size_t* lds_bytes) {
  std::lock_guard<std::mutex> lk(g_llog_mu);
  if (i < 0 || i >= (int)g_llog_recs.size() || !name || !variant || !rb || !ntiles || !grid || !block || !lds_bytes) return FNO_EINVAL;
  const LaunchRec& r = g_llog_recs[i];
  *name = r.name; *variant = r.tag.variant ? r.tag.variant : ""; *rb = r.tag.rb; *ntiles = r.tag.ntiles; *lds_bytes = r.lds;
  for (int d = 0; d < 3; ++d) { grid[d] = r.grid[d]; block[d] = r.block[d]; }
  return FNO_OK;
}

#ifdef FNO_CLOCK
extern "C" int fno_debug_clock_dump(unsigned long long* host, size_t n) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_clk), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FNO_TRACE
extern "C" int fno_debug_trace_dump(unsigned long long* host, size_t n) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trace), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
// events come from a pool that survives fno_profile_reset(): creating two events per launch inside the profiled steps
// slows the host enough to leave gaps between the kernels (the measured durations then carry the ramp of an idle GPU)
static std::vector<hipEvent_t> g_evpool;
static size_t g_evused = 0;
static hipEvent_t prof_event() {
  if (g_evused == g_evpool.size()) {
    hipEvent_t e;
    hipEventCreate(&e);
    g_evpool.push_back(e);
  }
  return g_evpool[g_evused++];
}
extern "C" void fno_profile_enable(int on) { g_prof = on != 0; }
extern "C" void fno_profile_reset(void) {
  g_recs.clear();
  g_agg.clear();
  g_evused = 0;
}
static void prof_aggregate() {
  if (g_recs.empty()) return;
  std::map<std::string, size_t> idx;
  for (auto& r : g_recs) {
    hipEventSynchronize(r.b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.a, r.b);
    auto it = idx.find(r.name);
    if (it == idx.end()) { idx[r.name] = g_agg.size(); g_agg.push_back({r.name, ms, 1, r.terms}); }
    else { g_agg[it->second].ms += ms; g_agg[it->second].n += 1; if (r.terms > g_agg[it->second].terms) g_agg[it->second].terms = r.terms; }
  }
  g_recs.clear();
  g_evused = 0;
}
extern "C" int fno_profile_count(void) { prof_aggregate(); return (int)g_agg.size(); }
extern "C" int fno_profile_get_terms(int i) {
  prof_aggregate();
  return (i < 0 || i >= (int)g_agg.size()) ? 0 : g_agg[i].terms;      // (0 = "not stated": never an error code as a term count)
}
extern "C" int fno_profile_get(int i, const char** name, float* total_ms, int* launches) {
  prof_aggregate();
  if (i < 0 || i >= (int)g_agg.size()) return FNO_EINVAL;
  *name = g_agg[i].name.c_str();
  *total_ms = g_agg[i].ms;
  *launches = g_agg[i].n;
  return FNO_OK;
}

static const int g_print_occ = getenv("FNO_PRINT_OCC") ? 1 : 0;
template <typename... KArgs, typename... Args>
static int launch(const char* name, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                  Args... args) {
  const int terms = g_terms_next;      // read and cleared before any early return: a failed launch must not leave it for the next one
  g_terms_next = 0;
  const LaunchTag tag = g_tag_next;
  g_tag_next = LaunchTag{nullptr, 0, 0};
  if (grid.x == 0 || grid.y == 0 || grid.z == 0) return FNO_OK;
  if (lds > 64 * 1024) {
    if (lds > FNO_LDS_MAX) return fail(FNO_EUNSUPPORTED, "%s needs %zu bytes of LDS (160 KB per CU)", name, lds);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();      // do not leave a sticky error for the next launch
      return fail(FNO_EHIP, "%s: set LDS %zu: %s", name, lds, hipGetErrorString(e));
    }
  }
  if (g_print_occ) {        // FNO_PRINT_OCC=1: resident workgroups per CU the runtime reports, once per kernel instantiation
    static std::map<const void*, int> seen;
    const void* key = reinterpret_cast<const void*>(kern);
    if (!seen.count(key)) {
      int nb = -1;
      hipFuncAttributes fa;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, (int)(block.x * block.y * block.z), lds);
      (void)hipFuncGetAttributes(&fa, key);
      seen[key] = nb;
      fprintf(stderr, "[occ] %-22s threads=%4u grid=%6u lds=%6zu+%zu regs=%3d -> %d workgroups/CU\n", name,
              block.x * block.y * block.z, grid.x * grid.y * grid.z, lds, (size_t)fa.sharedSizeBytes, fa.numRegs, nb);
    }
  }
  ProfRec rec;
  if (g_prof) {
    rec.name = name;
    rec.terms = terms;
    rec.a = prof_event();
    rec.b = prof_event();
    hipEventRecord(rec.a, st);
  }
  if (g_llog) {
    std::lock_guard<std::mutex> lk(g_llog_mu);
    g_llog_recs.push_back(LaunchRec{name, tag, {grid.x, grid.y, grid.z}, {block.x, block.y, block.z}, lds});
  }
  hipLaunchKernelGGL(kern, grid, block, lds, st, static_cast<KArgs>(args)...);
  hipError_t e = hipGetLastError();
  if (g_prof) { hipEventRecord(rec.b, st); g_recs.push_back(rec); }
  if (e != hipSuccess) return fail(FNO_EHIP, "launch %s: %s", name, hipGetErrorString(e));
  return FNO_OK;
}
#define LAUNCHCHK(expr) do { int rc_ = (expr); if (rc_ != FNO_OK) return rc_; } while (0)

// --------------------------------------------------------------------------
// geometry + tables shared by both plan kinds
// --------------------------------------------------------------------------
struct Geom {
  int ndim, nlead;
  int dims[3];
  int modes[3];
  int W, P, PW;
  int Klead[2];   // 2*modes on the leading dims
  int Klast, J, NJ;
  int Ktot;
  int wl_stride;
  int w_planes;      // corner weights stored plane-major ([wl][Cin][Cout][rest], k_spectral_mid.h)
  double s_f, s_i;
};

struct Tables {
  float* tfwd_f = nullptr;   // (16*NJ, W)  cos / -sin
  float* tfwd_b = nullptr;   // same, gamma-weighted (transform of gradients)
  float* tinv_f = nullptr;   // (J, W) gamma * s_i * (cos, -sin)
  float* tinv_b = nullptr;   // (J, W) s_f * (cos, -sin)
  float* tT[4] = {nullptr, nullptr, nullptr, nullptr};   // tfwd_f, tfwd_b, tinv_f, tinv_b transposed to [W][2*K2P], zero-padded bins
  int K2P = 0;               // kept bins rounded up to 8 / 16 / 32 (0: more than 32, no transposed tables)
  float2* tw_fwd_sf[2] = {nullptr, nullptr};  // leading dim d: TRANSPOSED (N, Klead) e^{-i}, d==0 scaled by s_f
  float2* tw_fwd_si[2] = {nullptr, nullptr};  // d==0 scaled by s_i (gradient direction)
  float2* tw_inv[2] = {nullptr, nullptr};     // (N, Klead) e^{+i}
  std::vector<void*> owned;
  void release() { for (void* p : owned) hipFree(p); owned.clear(); }
};

static int upload(Tables& t, const void* host, size_t bytes, void** dev) {
  HIPCHK(hipMalloc(dev, bytes));
  t.owned.push_back(*dev);
  HIPCHK(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
  return FNO_OK;
}

// allow_1d: the standalone spectral convolution has one-dimensional kernels (k_spec1d.h); the whole-model plan has none
static int make_geom(Geom& g, int ndim, const int* dims, const int* modes, int wl_stride, int norm, int w_planes = 0,
                     bool allow_1d = false) {
  if (ndim != 2 && ndim != 3 && !(allow_1d && ndim == 1))
    return fail(FNO_EUNSUPPORTED, allow_1d ? "ndim=%d (1, 2 or 3 supported)" : "ndim=%d (2 or 3 supported)", ndim);
  g.ndim = ndim;
  g.nlead = ndim - 1;
  g.PW = 1;
  for (int d = 0; d < ndim; ++d) {
    g.dims[d] = dims[d];
    g.modes[d] = modes[d];
    if (dims[d] < 1 || modes[d] < 1) return fail(FNO_EINVAL, "dims/modes must be >= 1");
    g.PW *= dims[d];
  }
  g.W = dims[ndim - 1];
  g.P = g.PW / g.W;
  g.Klast = modes[ndim - 1];
  if (g.Klast > g.W / 2 + 1) return fail(FNO_EINVAL, "modes[last]=%d exceeds W/2+1=%d", g.Klast, g.W / 2 + 1);
  g.Ktot = g.Klast;
  for (int d = 0; d < g.nlead; ++d) {
    if (modes[d] > dims[d]) return fail(FNO_EINVAL, "modes[%d]=%d exceeds dims=%d", d, modes[d], dims[d]);
    // Overlapping corners (2 m > N).  The reference assigns the corners in order into one zero-filled spectrum
    // (spectral_convolution.py:330-337, rno.py:71-74, basics.py:86-89): rows that belong to both take the SECOND corner's
    // product, and the first corner's weights at those rows see neither data nor gradient.  One leading dim: the first
    // corner's shadowed slots are switched off in the two truncating tables (make_tables) - nothing else changes, every
    // kernel keeps its 2 m slots.  Two leading dims (four corners, three assignment orders to restate): still refused.
    if (2 * modes[d] > dims[d] && g.nlead != 1)
      return fail(FNO_EUNSUPPORTED, "overlapping corners: 2*modes[%d]=%d > dims=%d (supported on 2-D grids)", d, 2 * modes[d], dims[d]);
    g.Klead[d] = 2 * modes[d];
    g.Ktot *= g.Klead[d];
  }
  g.J = 2 * g.Klast;
  g.NJ = (g.J + 15) / 16;
  g.wl_stride = wl_stride > 0 ? wl_stride : g.Klast;
  if (g.wl_stride < g.Klast) return fail(FNO_EINVAL, "weight_last_extent < modes[last]");
  g.w_planes = w_planes ? 1 : 0;
  const double n = (double)g.PW;
  if (norm == FNO_NORM_FORWARD) { g.s_f = 1.0 / n; g.s_i = 1.0; }
  else if (norm == FNO_NORM_ORTHO) { g.s_f = 1.0 / std::sqrt(n); g.s_i = g.s_f; }
  else if (norm == FNO_NORM_BACKWARD) { g.s_f = 1.0; g.s_i = 1.0 / n; }
  else return fail(FNO_EINVAL, "norm=%d", norm);
  return FNO_OK;
}

static int make_tables(const Geom& g, Tables& t) {
  const double PI2 = 6.283185307179586476925286766559;
  const int W = g.W, J = g.J;
  std::vector<float> ff((size_t)16 * g.NJ * W, 0.f), fb((size_t)16 * g.NJ * W, 0.f);
  std::vector<float> vf((size_t)J * W), vb((size_t)J * W);
  for (int k2 = 0; k2 < g.Klast; ++k2) {
    const double gamma = (k2 == 0 || (W % 2 == 0 && k2 == W / 2)) ? 1.0 : 2.0;
    for (int w = 0; w < W; ++w) {
      const double ang = PI2 * (double)((long long)k2 * w % W) / W;
      const double c = std::cos(ang), s = std::sin(ang);
      ff[(size_t)(2 * k2) * W + w] = (float)c;
      ff[(size_t)(2 * k2 + 1) * W + w] = (float)(-s);
      fb[(size_t)(2 * k2) * W + w] = (float)(gamma * c);
      fb[(size_t)(2 * k2 + 1) * W + w] = (float)(-gamma * s);
      vf[(size_t)(2 * k2) * W + w] = (float)(gamma * g.s_i * c);
      vf[(size_t)(2 * k2 + 1) * W + w] = (float)(-gamma * g.s_i * s);
      vb[(size_t)(2 * k2) * W + w] = (float)(g.s_f * c);
      vb[(size_t)(2 * k2 + 1) * W + w] = (float)(-g.s_f * s);
    }
  }
  int rc;
  if ((rc = upload(t, ff.data(), ff.size() * 4, (void**)&t.tfwd_f))) return rc;
  if ((rc = upload(t, fb.data(), fb.size() * 4, (void**)&t.tfwd_b))) return rc;
  if ((rc = upload(t, vf.data(), vf.size() * 4, (void**)&t.tinv_f))) return rc;
  if ((rc = upload(t, vb.data(), vb.size() * 4, (void**)&t.tinv_b))) return rc;
  // (1-D plans: no kernel of k_spec1d.h reads the transposed tables - up to 4 x 2 MB at N = 8192 that a cached plan would hold)
  t.K2P = g.ndim == 1 ? 0 : g.Klast <= 8 ? 8 : g.Klast <= 16 ? 16 : g.Klast <= 32 ? 32 : 0;
  if (t.K2P) {
    const std::vector<float>* src[4] = {&ff, &fb, &vf, &vb};
    for (int q = 0; q < 4; ++q) {
      std::vector<float> tr((size_t)W * 2 * t.K2P, 0.f);
      for (int j = 0; j < J; ++j)
        for (int w = 0; w < W; ++w) tr[(size_t)w * 2 * t.K2P + j] = (*src[q])[(size_t)j * W + w];
      if ((rc = upload(t, tr.data(), tr.size() * 4, (void**)&t.tT[q]))) return rc;
    }
  }
  for (int d = 0; d < g.nlead; ++d) {
    const int N = g.dims[d], K = g.Klead[d], m = g.modes[d];
    std::vector<float2> a((size_t)K * N), b((size_t)K * N), inv((size_t)N * K);
    for (int r = 0; r < K; ++r) {
      const int freq = r < m ? r : N - 2 * m + r;
      // overlapping corners: slot r of the first corner is shadowed when the second corner holds the same row (make_geom)
      const bool shadowed = r < m && r >= N - m;
      for (int n = 0; n < N; ++n) {
        const double ang = PI2 * (double)((long long)freq * n % N) / N;
        const double c = std::cos(ang), s = std::sin(ang);
        const double sa = shadowed ? 0.0 : (d == 0 ? g.s_f : 1.0), sb = shadowed ? 0.0 : (d == 0 ? g.s_i : 1.0);
        a[(size_t)n * K + r] = make_float2((float)(sa * c), (float)(-sa * s));
        b[(size_t)n * K + r] = make_float2((float)(sb * c), (float)(-sb * s));
        inv[(size_t)n * K + r] = make_float2((float)c, (float)s);
      }
    }
    if ((rc = upload(t, a.data(), a.size() * 8, (void**)&t.tw_fwd_sf[d]))) return rc;
    if ((rc = upload(t, b.data(), b.size() * 8, (void**)&t.tw_fwd_si[d]))) return rc;
    if ((rc = upload(t, inv.data(), inv.size() * 8, (void**)&t.tw_inv[d]))) return rc;
  }
  return FNO_OK;
}

// workspace bump allocator (256-B aligned pieces)
struct Carver {
  char* base; size_t cap, off = 0; bool ok = true;
  Carver(void* b, size_t c) : base((char*)b), cap(c) {}
  template <typename T> T* take(size_t count) {
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    if (!base || off + bytes > cap) { ok = false; off += bytes; return nullptr; }
    T* p = (T*)(base + off);
    off += bytes;
    return p;
  }
};

static ModeMap make_modemap(const Geom& g, int Cin, int Cout) {
  ModeMap mm;
  mm.nlead = g.nlead;
  for (int d = 0; d < 3; ++d) { mm.K[d] = 1; mm.m[d] = 1; }
  for (int d = 0; d < g.nlead; ++d) { mm.K[d] = g.Klead[d]; mm.m[d] = g.modes[d]; }
  mm.K[g.nlead] = g.Klast;
  mm.m[g.nlead] = g.Klast;
  mm.wl_stride = g.wl_stride;
  mm.Cin = Cin; mm.Cout = Cout; mm.Ktot = g.Ktot;
  return mm;
}


// many -> few (twT transposed (n_in, n_out)) or few -> many (tw (n_out, n_in)); the small (kept) extent
// is a template parameter of the fast kernels (2*m for the usual m = 2..20), anything else is generic.
#define FNO_AXIS_GENERIC 1      // axis_pass_t: "take the generic kernel" (not an error code: those are negative)
// launch-log tags of axis_pass_t<NS>: form 0 k_axis_fwd<NS,SEGS,true>, 1 k_axis_fwd<NS,SEGS>, 2 k_axis_inv<NS,ISEGS,true>, 3 k_axis_inv<NS,ISEGS>
template <int NS>
static const char* axis_tag(int form) {
#define AXT(NS_) case NS_: { static const char* const t[4] = {"k_axis_fwd<" #NS_ ",tlds>", "k_axis_fwd<" #NS_ ">", "k_axis_inv<" #NS_ ",tlds>", "k_axis_inv<" #NS_ ">"}; return t[form]; }
  switch (NS) { AXT(4) AXT(6) AXT(8) AXT(10) AXT(12) AXT(16) AXT(24) AXT(32) AXT(40) }
#undef AXT
  return "k_axis<?>";
}
template <int NS>
static int axis_pass_t(hipStream_t st, bool truncating, const float2* in, float2* out, const float2* tw, int outer,
                       int n_in, int n_out, int inner) {
  constexpr int SEGS = NS > 24 ? 4 : 8;      // partial sums [SEGS][NS][64] complex: 80 KB at NS = 40
  // (>= 24 kept modes read their twiddle table from LDS instead of the scalar cache: k_axis_fwd<40> 0.47 -> 0.30 ms, round 1;
  // `if constexpr`: the LDS-table variants of the smaller mode counts are not compiled)
  if (truncating) {
    const size_t red = (size_t)SEGS * NS * 64 * 8, tab = (size_t)n_in * NS * 8;
    if constexpr (NS >= 24) {
      if (std::max(red, tab) > 96 * 1024) return FNO_AXIS_GENERIC;      // (sweeps of > 300 rows: the generic kernel)
      return LV(axis_tag<NS>(0), 0, 0), launch("k_axis_fwd_tlds", k_axis_fwd<NS, SEGS, true>, dim3((inner + 63) / 64, outer), dim3(64, SEGS), std::max(red, tab), st,
                    in, out, tw, n_in, inner);
    } else
    return LV(axis_tag<NS>(1), 0, 0), launch("k_axis_fwd", k_axis_fwd<NS, SEGS>, dim3((inner + 63) / 64, outer), dim3(64, SEGS), red, st, in, out, tw, n_in,
                  inner);
  }
  constexpr int ISEGS = NS > 24 ? 8 : 16;
  if constexpr (NS >= 24) {
    if ((size_t)n_out * NS * 8 > 96 * 1024) return FNO_AXIS_GENERIC;
    return LV(axis_tag<NS>(2), 0, 0), launch("k_axis_inv_tlds", k_axis_inv<NS, ISEGS, true>, dim3((inner + 63) / 64, outer), dim3(64, ISEGS), (size_t)n_out * NS * 8,
                  st, in, out, tw, n_out, inner);
  } else
  return LV(axis_tag<NS>(3), 0, 0), launch("k_axis_inv", k_axis_inv<NS, ISEGS>, dim3((inner + 63) / 64, outer), dim3(64, ISEGS), 0, st, in, out, tw,
                n_out, inner);
}
static int axis_pass(hipStream_t st, bool truncating, const float* in_, float* out_, const float2* tw, int outer,
                     int n_in, int n_out, int inner) {
  if (outer > 65535) return fail(FNO_EUNSUPPORTED, "axis pass grid too large (%d)", outer);
  const float2* in = (const float2*)in_;
  float2* out = (float2*)out_;
  const int small = truncating ? n_out : n_in;
  int rc = FNO_AXIS_GENERIC;
  switch (small) {      // the kept extent is a template parameter of the fast kernels (2 m for m = 2, 3, 4, 5, 6, 8, 12, 16, 20)
    case 4: rc = axis_pass_t<4>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 6: rc = axis_pass_t<6>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 8: rc = axis_pass_t<8>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 10: rc = axis_pass_t<10>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 12: rc = axis_pass_t<12>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 16: rc = axis_pass_t<16>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 24: rc = axis_pass_t<24>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 32: rc = axis_pass_t<32>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;
    case 40: rc = axis_pass_t<40>(st, truncating, in, out, tw, outer, n_in, n_out, inner); break;   // modes 20: BASELINE config 5
    default: break;
  }
  if (rc != FNO_AXIS_GENERIC) return rc;
  if (n_out > 65535) return fail(FNO_EUNSUPPORTED, "axis pass grid too large (%d)", n_out);
  return LV(truncating ? "k_axis_generic(truncating)" : "k_axis_generic(extending)", 0, 0), launch("k_axis_generic", k_axis_generic, dim3((inner + 255) / 256, n_out, outer), dim3(256), 0, st, in, out,
                tw, n_in, n_out, inner, truncating ? 1 : 0);
}

// forward-direction passes over the leading dims: x1 [B][lead..][Klast][C] -> hat [B][K..][Klast][C]
static int lead_forward(hipStream_t st, const Geom& g, const Tables& t, bool grad_dir, int B, int C, const float* x1,
                        float* tmp, float* hat) {
  const float2* tw0 = grad_dir ? t.tw_fwd_si[0] : t.tw_fwd_sf[0];
  if (g.nlead == 1) return axis_pass(st, true, x1, hat, tw0, B, g.dims[0], g.Klead[0], g.Klast * C);
  LAUNCHCHK(axis_pass(st, true, x1, tmp, t.tw_fwd_sf[1], B * g.dims[0], g.dims[1], g.Klead[1], g.Klast * C));
  return axis_pass(st, true, tmp, hat, tw0, B, g.dims[0], g.Klead[0], g.Klead[1] * g.Klast * C);
}
// inverse passes: hat [B][K..][Klast][C] -> z [B][lead..][Klast][C]
static int lead_inverse(hipStream_t st, const Geom& g, const Tables& t, int B, int C, const float* hat, float* tmp,
                        float* z) {
  if (g.nlead == 1) return axis_pass(st, false, hat, z, t.tw_inv[0], B, g.Klead[0], g.dims[0], g.Klast * C);
  LAUNCHCHK(axis_pass(st, false, hat, tmp, t.tw_inv[0], B, g.Klead[0], g.dims[0], g.Klead[1] * g.Klast * C));
  return axis_pass(st, false, tmp, z, t.tw_inv[1], B * g.dims[0], g.Klead[1], g.dims[1], g.Klast * C);
}

// The fused middle (k_spec_mid): one leading dim, 32 / 64 channels, whole last-dim bins per 64-column workgroup, a kept
// leading extent with an instantiation.  FNO_NO_FUSED_MID=1 keeps the three-launch sequence (A/B switch).
static int g_fused_mid = getenv("FNO_NO_FUSED_MID") ? 0 : 1;
extern "C" void fno_set_fused_mid(int on) { g_fused_mid = on ? 1 : 0; }
extern "C" int fno_get_fused_mid(void) { return g_fused_mid; }
static bool fused_mid_shape_ok(const Geom& g, int C) {      // decides what the forward packs (the switch may flip before the backward)
  if (g.nlead != 1 || (C != 32 && C != 64) || (g.Klast * C) % 64 != 0) return false;
  if (g.dims[0] > 512) return false;             // the (n, Klead) tables are staged in the partial-sum region
  const int nk = g.Klead[0];
  // 24 kept modes: one workgroup per CU (123 KB of LDS), measured no faster than the three launches (RNO2d 128^2: 6.30 vs 6.26 ms)
  return nk == 4 || nk == 8 || nk == 12 || nk == 16;
}
static bool fused_mid_ok(const Geom& g, int C) { return g_fused_mid && fused_mid_shape_ok(g, C); }
template <int NK>
static int spec_mid_t(hipStream_t st, int C, const float2* x1, float2* hat, const float2* wm, float2* z, const float2* twT,
                      const float2* twi, int n, int inner, int K2, int conj_w, int samples, int Bm, size_t w_ms) {
  const size_t lds = (size_t)10 * NK * 64 * 8;
  const dim3 grid(inner / 64, samples), blk(64, 8);
  if (C == 32) return launch("k_spec_mid", k_spec_mid<NK, 32>, grid, blk, lds, st, x1, hat, wm, z, twT, twi, n, inner, K2, conj_w, Bm, w_ms);
  return launch("k_spec_mid", k_spec_mid<NK, 64>, grid, blk, lds, st, x1, hat, wm, z, twT, twi, n, inner, K2, conj_w, Bm, w_ms);
}
// x1 [samples][n][Klast][C] -> hat [samples][Klead][Klast][C] (kept for the weight gradient) and z [samples][n][Klast][C];
// wm: packed weights [k][i][o] (conj_w = 0) or their transposed copy [k][o][i] (conj_w = 1: the adjoint); sample s uses
// the weights of member s / Bm (w_ms floats apart)
static int spectral_mid_fused(hipStream_t st, const Geom& g, const Tables& t, bool grad_dir, int samples, int C,
                              const float* x1, float* hat, const float* wm, float* z, int conj_w, int Bm = 1 << 30,
                              size_t w_ms = 0) {
  if (samples > 65535) return fail(FNO_EUNSUPPORTED, "spectral middle grid too large (%d)", samples);
  const float2* twT = grad_dir ? t.tw_fwd_si[0] : t.tw_fwd_sf[0];
  const float2 *xx = (const float2*)x1, *ww = (const float2*)wm;
  float2 *hh = (float2*)hat, *zz = (float2*)z;
  const int n = g.dims[0], inner = g.Klast * C;
  switch (g.Klead[0]) {
    case 4: return spec_mid_t<4>(st, C, xx, hh, ww, zz, twT, t.tw_inv[0], n, inner, g.Klast, conj_w, samples, Bm, w_ms / 2);
    case 8: return spec_mid_t<8>(st, C, xx, hh, ww, zz, twT, t.tw_inv[0], n, inner, g.Klast, conj_w, samples, Bm, w_ms / 2);
    case 12: return spec_mid_t<12>(st, C, xx, hh, ww, zz, twT, t.tw_inv[0], n, inner, g.Klast, conj_w, samples, Bm, w_ms / 2);
    case 16: return spec_mid_t<16>(st, C, xx, hh, ww, zz, twT, t.tw_inv[0], n, inner, g.Klast, conj_w, samples, Bm, w_ms / 2);
  }
  return fail(FNO_EUNSUPPORTED, "fused spectral middle: %d kept leading modes", g.Klead[0]);
}

// nm > 1: nm independent contractions in one launch (fan-out members); *_ms = member strides in floats (0 = shared operand).
// Only the matrix-core kernels take members; callers check mode_gemm_members_ok() first.
static bool mode_gemm_members_ok(int Cin, int Cout) {
  return g_mode_mfma && Cin == Cout && (Cin == 32 || Cin == 64);      // (square blocks: what every model of the reference has)
}
static int mode_gemm(hipStream_t st, const float* x, const float* w, float* out, int B, int Ktot, int Cin, int Cout,
                     int conj_w, int nm = 1, size_t x_ms = 0, size_t w_ms = 0, size_t o_ms = 0, int trans_w = 0) {
  if (Cout > 256) return fail(FNO_EUNSUPPORTED, "channels > 256");
  if (trans_w && !mode_gemm_members_ok(Cin, Cout)) return fail(FNO_EUNSUPPORTED, "transposed-weight contraction needs the matrix-core kernels");
  if (g_mode_mfma && nm == 1 && B <= 4 && Cin <= 64 && Cout <= 64 && (long)Ktot * Cin * Cout >= (1L << 21)) {
    // tiny batch, many modes: a stream over the weights (k_mode_gemv*); x / out hold B samples back to back
    const float2 *xx = (const float2*)x, *ww = (const float2*)w;
    float2* oo = (float2*)out;
    if (!trans_w) {
      const dim3 grid((Ktot + 3) / 4), blk(256);
      switch (B) {
        case 1: return LV("k_mode_gemv<1>", 0, 0), launch("k_mode_gemv", k_mode_gemv<1>, grid, blk, 0, st, xx, ww, oo, Ktot, Cin, Cout, conj_w);
        case 2: return LV("k_mode_gemv<2>", 0, 0), launch("k_mode_gemv", k_mode_gemv<2>, grid, blk, 0, st, xx, ww, oo, Ktot, Cin, Cout, conj_w);
        case 3: return LV("k_mode_gemv<3>", 0, 0), launch("k_mode_gemv", k_mode_gemv<3>, grid, blk, 0, st, xx, ww, oo, Ktot, Cin, Cout, conj_w);
        default: return LV("k_mode_gemv<4>", 0, 0), launch("k_mode_gemv", k_mode_gemv<4>, grid, blk, 0, st, xx, ww, oo, Ktot, Cin, Cout, conj_w);
      }
    } else if (conj_w) {
      // here `Cin` counts the channels of x (= the forward's Cout) and the stored block is (Cout, Cin) = forward (Cin_f, Cout_f)
      const dim3 grid(Ktot), blk(256);
      const size_t lds = (size_t)Cout * (Cin + 1) * 8;
      switch (B) {
        case 1: return LV("k_mode_gemv_t<1>", 0, 0), launch("k_mode_gemv_t", k_mode_gemv_t<1>, grid, blk, lds, st, xx, ww, oo, Ktot, Cout, Cin);
        case 2: return LV("k_mode_gemv_t<2>", 0, 0), launch("k_mode_gemv_t", k_mode_gemv_t<2>, grid, blk, lds, st, xx, ww, oo, Ktot, Cout, Cin);
        case 3: return LV("k_mode_gemv_t<3>", 0, 0), launch("k_mode_gemv_t", k_mode_gemv_t<3>, grid, blk, lds, st, xx, ww, oo, Ktot, Cout, Cin);
        default: return LV("k_mode_gemv_t<4>", 0, 0), launch("k_mode_gemv_t", k_mode_gemv_t<4>, grid, blk, lds, st, xx, ww, oo, Ktot, Cout, Cin);
      }
    }
  }
  if (nm > 1 && !mode_gemm_members_ok(Cin, Cout)) return fail(FNO_EUNSUPPORTED, "batched mode contraction needs the matrix-core kernels");
  if (mode_gemm_members_ok(Cin, Cout)) {     // one real GEMM per mode on the matrix cores
    // batch rows per workgroup (k_spectral_mid.h): 32 where the batch has no more AND the workgroup stays four waves
    // (64 output channels; at 32 channels the two-wave workgroup stages its weights too slowly: 10.7 vs 8.6 us at FNO3d)
    const int br = (B > 32 || Cout < 64) ? 64 : 32;
    const dim3 grid(Ktot, (B + br - 1) / br, nm), blk((br / 32) * (2 * Cout / 32) * 64);
    const size_t lds = (size_t)br * (2 * Cin + 1) * 4 + (size_t)std::max(Cin * (Cout + 1), Cout * (Cin + 1)) * 8;      // spectra + the complex weight block
    const float2 *xx = (const float2*)x, *ww = (const float2*)w;
    float2* oo = (float2*)out;
    if (Cin == 32)      // (br = 64 always at 32 channels, above)
      return LV("k_mode_gemm_mfma<32,32,64>", br, 0), launch("k_mode_gemm", k_mode_gemm_mfma<32, 32, 64>, grid, blk, lds, st, xx, ww, oo, B, Ktot, conj_w, x_ms / 2, w_ms / 2, o_ms / 2, trans_w);
    if (br == 64) return LV("k_mode_gemm_mfma<64,64,64>", br, 0), launch("k_mode_gemm", k_mode_gemm_mfma<64, 64, 64>, grid, blk, lds, st, xx, ww, oo, B, Ktot, conj_w, x_ms / 2, w_ms / 2, o_ms / 2, trans_w);
    return LV("k_mode_gemm_mfma<64,64,32>", br, 0), launch("k_mode_gemm", k_mode_gemm_mfma<64, 64, 32>, grid, blk, lds, st, xx, ww, oo, B, Ktot, conj_w, x_ms / 2, w_ms / 2, o_ms / 2, trans_w);
  }
  if (512 % Cout == 0 && Cout >= 32) {
    const int bt = 2 * (512 / Cout);                   // 2 batch rows per thread
    const size_t lds = ((size_t)Cin * Cout + (size_t)bt * Cin) * 8;
    if (lds <= 150 * 1024)
      return LV("k_mode_gemm_lds<2>", bt, 0), launch("k_mode_gemm", k_mode_gemm_lds<2>, dim3(Ktot, (B + bt - 1) / bt), dim3(512), lds, st,
                    (const float2*)x, (const float2*)w, (float2*)out, B, Ktot, Cin, Cout, conj_w);
  }
  const int nb = 256 / Cout;
  dim3 grid(Ktot, (B + nb - 1) / nb);
  return LV("k_mode_gemm", nb, 0), launch("k_mode_gemm", k_mode_gemm, grid, dim3(256), 0, st, (const float2*)x, (const float2*)w, (float2*)out, B,
                Ktot, Cin, Cout, conj_w);
}
static int mode_gemm_dw(hipStream_t st, const float* x, const float* g, float* dw, int B, int Ktot, int Cin, int Cout,
                        int nm = 1, size_t x_ms = 0, size_t g_ms = 0, size_t d_ms = 0) {
  if (Cout > 256) return fail(FNO_EUNSUPPORTED, "channels > 256");
  if (nm > 1 && !mode_gemm_members_ok(Cin, Cout)) return fail(FNO_EUNSUPPORTED, "batched mode contraction needs the matrix-core kernels");
  if (g_mode_mfma && nm == 1 && B <= 4 && Cin <= 64 && Cout <= 64 && (long)Ktot * Cin * Cout >= (1L << 21)) {
    const dim3 grid((Ktot + 3) / 4), blk(256);
    const float2 *xx = (const float2*)x, *gg = (const float2*)g;
    float2* dd = (float2*)dw;
    switch (B) {
      case 1: return LV("k_mode_outer_dw<1>", 0, 0), launch("k_mode_outer_dw", k_mode_outer_dw<1>, grid, blk, 0, st, xx, gg, dd, Ktot, Cin, Cout);
      case 2: return LV("k_mode_outer_dw<2>", 0, 0), launch("k_mode_outer_dw", k_mode_outer_dw<2>, grid, blk, 0, st, xx, gg, dd, Ktot, Cin, Cout);
      case 3: return LV("k_mode_outer_dw<3>", 0, 0), launch("k_mode_outer_dw", k_mode_outer_dw<3>, grid, blk, 0, st, xx, gg, dd, Ktot, Cin, Cout);
      default: return LV("k_mode_outer_dw<4>", 0, 0), launch("k_mode_outer_dw", k_mode_outer_dw<4>, grid, blk, 0, st, xx, gg, dd, Ktot, Cin, Cout);
    }
  }
  if (mode_gemm_members_ok(Cin, Cout)) {
    const dim3 grid(Ktot, nm), blk((Cin / 32) * (2 * Cout / 32) * 64);
    const int bc = B > 32 ? 32 : 16;      // samples staged per chunk (k_spectral_mid.h)
    const size_t lds = ((size_t)bc * 2 * Cin + (size_t)2 * bc * (2 * Cout + 32)) * 4;
    const float2 *xx = (const float2*)x, *gg = (const float2*)g;
    float2* dd = (float2*)dw;
#define DWK(CI_, CO_) do { \
      if (bc == 32) return LV("k_mode_gemm_dw_mfma<" #CI_ "," #CO_ ",32>", bc, 0), launch("k_mode_gemm_dw", k_mode_gemm_dw_mfma<CI_, CO_, 32>, grid, blk, lds, st, xx, gg, dd, B, Ktot, x_ms / 2, g_ms / 2, d_ms / 2); \
      return LV("k_mode_gemm_dw_mfma<" #CI_ "," #CO_ ",16>", bc, 0), launch("k_mode_gemm_dw", k_mode_gemm_dw_mfma<CI_, CO_, 16>, grid, blk, lds, st, xx, gg, dd, B, Ktot, x_ms / 2, g_ms / 2, d_ms / 2); } while (0)
    if (Cin == 32) DWK(32, 32);
    DWK(64, 64);
#undef DWK
  }
  if (512 % Cout == 0 && Cout >= 32) {
    const int it = 2 * (512 / Cout);                   // 2 input channels per thread
    return LV("k_mode_gemm_dw_lds<2>", it, 0), launch("k_mode_gemm_dw", k_mode_gemm_dw_lds<2>, dim3(Ktot, (Cin + it - 1) / it), dim3(512),
                  (size_t)64 * (it + Cout) * 8, st, (const float2*)x, (const float2*)g, (float2*)dw, B, Ktot, Cin, Cout);
  }
  const int ni = 256 / Cout;
  dim3 grid(Ktot, (Cin + ni - 1) / ni);
  return LV("k_mode_gemm_dw", ni, 0), launch("k_mode_gemm_dw", k_mode_gemm_dw, grid, dim3(256), 0, st, (const float2*)x, (const float2*)g,
                (float2*)dw, B, Ktot, Cin, Cout);
}
// all layers of a stack in one launch each way (blockIdx.y = layer); wp / wpt nullable; `stride` = floats between layers
static int nrest_of(const Geom& g) { return g.nlead == 2 ? g.modes[0] * g.modes[1] : g.modes[0]; }
static int plane_rc(int nrest) { int rc = 64; while (rc > 8 && rc / 2 >= nrest) rc >>= 1; return rc; }      // rest positions per tile
static size_t plane_blocks(const Geom& g, int Cin, int Cout, int nrest, int rc) {
  return (size_t)(1 << g.nlead) * g.Klast * ((Cin + 7) / 8) * ((Cout + 7) / 8) * ((nrest + rc - 1) / rc);
}
// zero64 (or null): kNAmax bound slots to clear before anything behind this launch runs (the tiled kernel does it itself)
static int pack_w_layers(hipStream_t st, const Geom& g, int Cin, int Cout, const CornerPtrsL& cp, int L, float* wp, float* wpt,
                         size_t stride, float* zero64 = nullptr) {
  const ModeMap mm = make_modemap(g, Cin, Cout);
  const int nrest = nrest_of(g);
  if (g.w_planes) {
    if (zero64 && hipMemsetAsync(zero64, 0, 64 * sizeof(float), st) != hipSuccess) return fail(FNO_EHIP, "memset of the magnitude bounds");
    const int rc = plane_rc(nrest);
    const size_t blocks = plane_blocks(g, Cin, Cout, nrest, rc);
    if (blocks > 0x7fffffffull) return fail(FNO_EUNSUPPORTED, "weight pack grid too large");
    return launch("k_pack_w", k_pack_w_planes, dim3((unsigned)blocks, L), dim3(256), (size_t)64 * (rc + 1) * 8, st, cp, (float2*)wp,
                  (float2*)wpt, mm, stride / 2, nrest, rc);
  }
  int ti = 8;                                  // input channels per workgroup: whole sectors of the transposed copy
  while (ti > 1 && (Cin % ti != 0 || (size_t)ti * Cout * (g.wl_stride + 1) * 8 > 48 * 1024)) ti >>= 1;   // >= 3 workgroups per CU
  const size_t blocks = (size_t)(1 << g.nlead) * nrest * (Cin / ti);
  if (blocks > 0x7fffffffull) return fail(FNO_EUNSUPPORTED, "weight pack grid too large");
  return launch("k_pack_w", k_pack_w_tiled, dim3((unsigned)blocks, L), dim3(256), (size_t)ti * Cout * (g.wl_stride + 1) * 8, st, cp,
                (float2*)wp, (float2*)wpt, mm, stride / 2, nrest, ti, zero64);
}
static int unpack_dw_layers(hipStream_t st, const Geom& g, int Cin, int Cout, const float* dwp, const CornerPtrsMutL& cp, int L,
                            size_t stride) {
  const ModeMap mm = make_modemap(g, Cin, Cout);
  const int nrest = nrest_of(g);
  if (g.w_planes) {
    const int rc = plane_rc(nrest);
    const size_t pblocks = plane_blocks(g, Cin, Cout, nrest, rc);
    if (pblocks > 0x7fffffffull) return fail(FNO_EUNSUPPORTED, "weight unpack grid too large");
    return launch("k_unpack_dw", k_unpack_dw_planes, dim3((unsigned)pblocks, L), dim3(256), (size_t)64 * (rc + 1) * 8, st,
                  (const float2*)dwp, cp, mm, stride / 2, nrest, rc);
  }
  const size_t blocks = (size_t)(1 << g.nlead) * nrest * Cin;
  if (blocks > 0x7fffffffull) return fail(FNO_EUNSUPPORTED, "weight unpack grid too large");
  return launch("k_unpack_dw", k_unpack_dw_tiled, dim3((unsigned)blocks, L), dim3(256), (size_t)Cout * (g.wl_stride + 1) * 8, st,
                (const float2*)dwp, cp, mm, stride / 2, nrest);
}
static int pack_w(hipStream_t st, const Geom& g, int Cin, int Cout, const float* const* corners, float* wp, float* wpt) {
  CornerPtrsL cpl;
  memset(&cpl, 0, sizeof(cpl));
  for (int c = 0; c < (1 << g.nlead); ++c) cpl.p[0][c] = (const float2*)corners[c];
  return pack_w_layers(st, g, Cin, Cout, cpl, 1, wp, wpt, 0);
}
static int unpack_dw(hipStream_t st, const Geom& g, int Cin, int Cout, const float* dwp, float* const* dcorners) {
  CornerPtrsMutL cpl;
  memset(&cpl, 0, sizeof(cpl));
  for (int c = 0; c < (1 << g.nlead); ++c) cpl.p[0][c] = (float2*)dcorners[c];
  return unpack_dw_layers(st, g, Cin, Cout, dwp, cpl, 1, 0);
}
static int reduce_slabs(hipStream_t st, const float* part, float* out, int nslab, int rows, int ncols, int ld_in,
                        int ld_out) {
  const int n = rows * ncols;
  return launch("k_reduce_slabs", k_reduce_slabs, dim3((n + 63) / 64), dim3(64, 16), 0, st, part, out, nslab, n,
                ld_out, ncols, ld_in);
}

struct JobList {
  ReduceJobs jobs;
  JobList() { jobs.count = 0; }
  void add(const float* part, float* out, int nslab, int rows, int ncols, int ld_in, int ld_out) {
    ReduceJob& j = jobs.j[jobs.count++];
    j.part = part; j.out = out; j.nslab = nslab; j.n = rows * ncols; j.ld_out = ld_out; j.ncols = ncols; j.ld_in = ld_in;
  }
  int run(hipStream_t st) {
    if (jobs.count == 0) return FNO_OK;
    return launch("k_reduce_jobs", k_reduce_jobs<64>, dim3(256, jobs.count), dim3(16, 64), 0, st, jobs);
  }
};

// ==========================================================================
// standalone spectral convolution
// ==========================================================================
struct FnoSpecPlan {
  FnoSpecDesc d;
  Geom g;
  Tables t;
};

static bool row_chan_ok(const Geom& g, int K2P, int C) { return K2P && C <= 64 && g.W <= 320; }
// the limits of the one-dimensional kernels (k_spec1d.h), each refused under its own name before any HIP call
static int spec1d_check(const FnoSpecDesc* d) {
  const int N = d->dims[0], M = d->modes[0];
  if ((d->Cin != 32 && d->Cin != 64) || (d->Cout != 32 && d->Cout != 64))
    return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: channels Cin=%d, Cout=%d (each 32 or 64)", d->Cin, d->Cout);
  if (N < 128 || N > 8192 || N % 128 != 0)
    return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: dims[0]=%d (a multiple of 128 in [128, 8192])", N);
  // (M <= 64 <= N / 2: the Nyquist bin is never kept)
  if (M < 1 || M > 64) return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: modes[0]=%d (1..64 kept bins, below the Nyquist bin)", M);
  if (d->weight_planes) return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: weight_planes=1 (plane-major weights are a 3-D layout)");
  return FNO_OK;
}
extern "C" int fno_spec_plan_create(const FnoSpecDesc* d, FnoSpecPlan** out) {
  if (!d || !out) return fail(FNO_EINVAL, "null argument");
  if (d->ndim == 1) {
    const int rc1 = spec1d_check(d);
    if (rc1 != FNO_OK) return rc1;
  }
  FnoSpecPlan* p = new FnoSpecPlan();
  p->d = *d;
  int rc = make_geom(p->g, d->ndim, d->dims, d->modes, d->weight_last_extent, d->norm, d->weight_planes, true);
  if (rc == FNO_OK && (d->Cin < 1 || d->Cout < 1 || d->Cin > 256 || d->Cout > 256))
    rc = fail(FNO_EUNSUPPORTED, "channels must be in [1, 256]");
  if (rc == FNO_OK && d->ndim != 1) {      // (1-D: the "row" is the whole sample and is cut into slabs, nothing to hold in LDS)
    const size_t lds1 = (size_t)std::max(d->Cin, d->Cout) * (p->g.W + 1) * 4;
    if (lds1 > FNO_LDS_MAX) rc = fail(FNO_EUNSUPPORTED, "row tile C*(W+1)*4=%zu exceeds LDS", lds1);
  }
  if (rc == FNO_OK) rc = make_tables(p->g, p->t);
  if (rc == FNO_OK && d->ndim != 1 && d->input_gelu && !row_chan_ok(p->g, p->t.K2P, d->Cin))
    rc = fail(FNO_EUNSUPPORTED, "input_gelu needs <= 64 input channels, rows of <= 320 floats and <= 32 kept last-dim bins");
  if (rc != FNO_OK) { p->t.release(); delete p; return rc; }
  *out = p;
  return FNO_OK;
}
extern "C" void fno_spec_plan_destroy(FnoSpecPlan* p) {
  if (!p) return;
  p->t.release();
  delete p;
}

// ---- one-dimensional grids (k_spec1d.h): analysis -> mix -> synthesis, three launches per direction ----
struct Spec1dWs { float *part, *hat, *dbpart, *xhat; size_t total; };
static Spec1dWs carve_spec1d(const FnoSpecPlan* p, int B, void* ws, size_t cap, bool* ok) {
  const int Cm = std::max(p->d.Cin, p->d.Cout), N = p->g.W, J = p->g.J, T = (N + S1_TILE - 1) / S1_TILE;
  Carver c(ws, cap);
  Spec1dWs w;
  w.part = c.take<float>((size_t)B * T * J * Cm);      // partial spectra of the slabs
  w.hat = c.take<float>((size_t)B * J * Cm);           // the mixed spectrum the synthesis reads
  w.dbpart = c.take<float>((size_t)B * T * Cm);        // slab sums of dy
  w.xhat = c.take<float>((size_t)B * J * p->d.Cin);    // the input spectrum of a forward that saves nothing
  w.total = c.off;
  if (ok) *ok = c.ok;
  return w;
}
static int spec1d_ana(hipStream_t st, int C, int B, int T, const float* x, const float* tab, float* part, float* dbpart, int N,
                      int J, int act) {
  const dim3 grid(T, B), blk(256);
  const size_t lds = (size_t)C * S1_TILE * 4;
  if (C == 32) return LV("k_s1_ana<32>", 0, T * B), launch("k_s1_ana", k_s1_ana<32>, grid, blk, lds, st, x, tab, part, dbpart, N, J, act);
  return LV("k_s1_ana<64>", 0, T * B), launch("k_s1_ana", k_s1_ana<64>, grid, blk, lds, st, x, tab, part, dbpart, N, J, act);
}
static int spec1d_syn(hipStream_t st, int C, int B, int T, const float* hat, const float* tab, const float* bias, float* y, int N,
                      int J) {
  const dim3 grid(T, B), blk(256);
  const size_t lds = (size_t)J * C * 4;
  if (C == 32) return LV("k_s1_syn<32>", 0, T * B), launch("k_s1_syn", k_s1_syn<32>, grid, blk, lds, st, hat, tab, bias, y, N, J);
  return LV("k_s1_syn<64>", 0, T * B), launch("k_s1_syn", k_s1_syn<64>, grid, blk, lds, st, hat, tab, bias, y, N, J);
}
static size_t spec_xhat_floats(const FnoSpecPlan* p, int B);
static int spec1d_forward(const FnoSpecPlan* p, hipStream_t st, int B, const float* x, const float* w0, const float* bias, float* y,
                          float* xhat_save, void* ws, size_t ws_bytes) {
  const Geom& g = p->g;
  const int Cin = p->d.Cin, Cout = p->d.Cout, N = g.W, M = g.Klast, J = g.J, T = (N + S1_TILE - 1) / S1_TILE;
  if (!w0) return fail(FNO_EINVAL, "fno_spec_forward: null corner weight");
  if (B > 65535) return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: batch %d (at most 65535)", B);
  bool ok;
  Spec1dWs w = carve_spec1d(p, B, ws, ws_bytes, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  LAUNCHCHK(spec1d_ana(st, Cin, B, T, x, p->t.tfwd_f, w.part, nullptr, N, J, p->d.input_gelu));
  const S1Weights sw{(const float2*)w0, Cout * g.wl_stride, g.wl_stride, 1};
  const size_t lds = ((size_t)Cin * (Cout + 1) + 16 * Cin) * 8;
  LAUNCHCHK((LV("k_s1_mix_fwd", 16, 0), launch("k_s1_mix", k_s1_mix_fwd, dim3(M, (B + 15) / 16), dim3(256), lds, st, w.part, sw,
                   (float2*)(xhat_save ? xhat_save : w.xhat), (float2*)(xhat_save ? xhat_save + spec_xhat_floats(p, B) : nullptr),
                   w.hat, B, T, M, Cin, Cout, (float)g.s_f)));
  return spec1d_syn(st, Cout, B, T, w.hat, p->t.tinv_f, bias, y, N, J);
}
static int spec1d_backward(const FnoSpecPlan* p, hipStream_t st, int B, const float* dy, const float* xhat, const float* w0,
                           float* dx, float* dw0, float* dbias, void* ws, size_t ws_bytes) {
  const Geom& g = p->g;
  const int Cin = p->d.Cin, Cout = p->d.Cout, N = g.W, M = g.Klast, J = g.J, T = (N + S1_TILE - 1) / S1_TILE;
  if (B > 65535) return fail(FNO_EUNSUPPORTED, "1-D spectral convolution: batch %d (at most 65535)", B);
  bool ok;
  Spec1dWs w = carve_spec1d(p, B, ws, ws_bytes, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  if (!dx && !dw0 && !dbias) return FNO_OK;
  LAUNCHCHK(spec1d_ana(st, Cout, B, T, dy, p->t.tfwd_b, w.part, dbias ? w.dbpart : nullptr, N, J, 0));
  // the weights for dx: the packed copy behind the saved spectrum, else the caller's tensor
  S1Weights sw{(const float2*)w0, Cout * g.wl_stride, g.wl_stride, 1};
  if (xhat) sw = S1Weights{(const float2*)(xhat + spec_xhat_floats(p, B)), Cout, 1, Cin * Cout};
  const size_t lds = ((size_t)Cin * (Cout + 1) + 8 * Cout + 8 * Cin) * 8;
  LAUNCHCHK((LV("k_s1_mix_bwd", 8, 0), launch("k_s1_mix", k_s1_mix_bwd, dim3(M), dim3(256), lds, st, w.part, (const float2*)xhat, sw,
                   (float2*)dw0, g.wl_stride, dx ? w.hat : nullptr, w.dbpart, dbias, B, T, M, Cin, Cout, (float)g.s_i)));
  if (!dx) return FNO_OK;
  return spec1d_syn(st, Cin, B, T, w.hat, p->t.tinv_b, nullptr, dx, N, J);
}

struct SpecWs {
  float *x1, *tmp, *hat_in, *hat_out, *z, *wp, *wpt, *dwp, *dbpart;
  size_t total;
};
static SpecWs carve_spec(const FnoSpecPlan* p, int B, void* ws, size_t cap, bool* ok) {
  const Geom& g = p->g;
  const int Cm = std::max(p->d.Cin, p->d.Cout);
  Carver c(ws, cap);
  SpecWs w;
  const size_t n_x1 = (size_t)B * g.P * g.Klast * Cm * 2;
  const size_t n_hat = (size_t)B * g.Ktot * Cm * 2;
  const size_t n_tmp = g.nlead == 2 ? (size_t)B * g.dims[0] * g.Klead[1] * g.Klast * Cm * 2 : 1;
  const size_t n_wp = (size_t)g.Ktot * p->d.Cin * p->d.Cout * 2;
  w.x1 = c.take<float>(n_x1);
  w.tmp = c.take<float>(n_tmp);
  w.hat_in = c.take<float>(n_hat);
  w.hat_out = c.take<float>(n_hat);
  w.z = c.take<float>(n_x1);
  w.wp = c.take<float>(n_wp);
  w.wpt = c.take<float>(n_wp);
  w.dwp = c.take<float>(n_wp);
  w.dbpart = c.take<float>((size_t)64 * Cm);
  w.total = c.off;
  if (ok) *ok = c.ok;
  return w;
}
extern "C" size_t fno_spec_workspace_bytes(const FnoSpecPlan* p, int B) {
  if (p->g.ndim == 1) return carve_spec1d(p, B, nullptr, 0, nullptr).total;
  return carve_spec(p, B, nullptr, 0, nullptr).total;
}
// saved for the backward: the truncated input spectrum [B][Ktot][Cin] and the transposed packed weights [Ktot][Cout][Cin]
static size_t spec_xhat_floats(const FnoSpecPlan* p, int B) { return (size_t)B * p->g.Ktot * p->d.Cin * 2; }
extern "C" size_t fno_spec_xhat_bytes(const FnoSpecPlan* p, int B) {
  return (spec_xhat_floats(p, B) + (size_t)p->g.Ktot * p->d.Cin * p->d.Cout * 2) * sizeof(float);
}

// Last-dim passes of the standalone path: MFMA tile kernels when the shape allows it
// (32 / 64 channels, rows of 32 / 64 / 128 floats, whole 128-pixel tiles), generic kernels otherwise.
static bool row_fast_ok(const Geom& g, int C) {
  return (C == 32 || C == 64) && g.W % 32 == 0 && 128 % g.W == 0 && g.PW % 128 == 0 && g.NJ <= 4;
}
static int dev_ncu() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
  }
  return ncu;
}
// what the tile kernel does to the rows while it stages them (k_rowdft_tile's MOD): dropout of the input, or the ReLU
// derivative read off a forward output (the masked tensor is written out as well)
struct RowMod { const unsigned* drop_seed = nullptr; float drop_p = 0.f; const float* ymask = nullptr; float* gmasked = nullptr; };
static int row_forward(hipStream_t st, const Geom& g, const float* tfwd, const float* tT, int K2P, int B, int C,
                       const float* x, float* x1, int act_in = 0, const RowMod* mod = nullptr) {
  if (act_in && !row_chan_ok(g, K2P, C)) return fail(FNO_EUNSUPPORTED, "input_gelu needs <= 64 channels, rows <= 320, <= 32 kept bins");
  if (mod && (act_in || !row_fast_ok(g, C))) return fail(FNO_EUNSUPPORTED, "dropout / ReLU-mask row passes need the tile kernel's shapes");
  if (!act_in && row_fast_ok(g, C)) {
    RowDftArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.x1 = x1; a.tfwd = tfwd; a.PW = g.PW; a.W = g.W; a.P = g.P; a.K2out = g.Klast; a.NJ = g.NJ;
    a.tiles_per_plane = g.PW / 128; a.ntiles = B * a.tiles_per_plane;
    const size_t lds = ((size_t)C * 132 + (size_t)16 * g.NJ * (g.W + 4)) * 4;
    const int grid = std::min(a.ntiles, 3 * dev_ncu());
    if (mod && mod->ymask) {
      a.ymask = mod->ymask; a.gmasked = mod->gmasked;
      if (C == 32) return launch("k_rowdft_tile_relu", k_rowdft_tile<32, 128, 2>, dim3(grid), dim3(256), lds, st, a);
      return launch("k_rowdft_tile_relu", k_rowdft_tile<64, 128, 2>, dim3(grid), dim3(256), lds, st, a);
    }
    if (mod && mod->drop_seed) {
      a.drop_seed = mod->drop_seed; a.drop_p = mod->drop_p;
      if (C == 32) return launch("k_rowdft_tile_drop", k_rowdft_tile<32, 128, 1>, dim3(grid), dim3(256), lds, st, a);
      return launch("k_rowdft_tile_drop", k_rowdft_tile<64, 128, 1>, dim3(grid), dim3(256), lds, st, a);
    }
    if (C == 32) return LV("k_rowdft_tile<32,128>", 0, a.ntiles), launch("k_rowdft_tile", k_rowdft_tile<32, 128>, dim3(grid), dim3(256), lds, st, a);
    return LV("k_rowdft_tile<64,128>", 0, a.ntiles), launch("k_rowdft_tile", k_rowdft_tile<64, 128>, dim3(grid), dim3(256), lds, st, a);
  }
  constexpr int chan_rb = 320;
  if (K2P) {
    // long 16-byte-aligned runs when the rows allow it: 8 channels x rb rows, rb * W % 4 == 0, P % rb == 0
    if (C % 8 == 0) {
      const int q = (g.W % 4 == 0) ? 1 : (g.W % 2 == 0 ? 2 : 4);            // rows per 16-byte period
      const int tabf = 2 * K2P * rowdft4_pitch((g.W + 3) & ~3) + 4;         // table + slack floats in the same LDS
      int rb = std::min(2560 / g.W, (int)(((80 * 1024 / 4 - tabf) / 8 - 36) / g.W)) / q * q;
      while (rb >= q && (g.P % rb != 0 || (long)B * (C / 8) * (g.P / rb) < 4L * dev_ncu())) rb -= q;
      if (rb >= q && rb * g.W >= 256) {
        const size_t lds = ((size_t)8 * rowdft4_pitch(rb * g.W) + 4 + (size_t)2 * K2P * rowdft4_pitch((g.W + 3) & ~3)) * 4;
        const int ntiles = B * (C / 8) * (g.P / rb);
        const int per_cu = std::max(1, (int)std::min<size_t>(4, FNO_LDS_MAX / lds));
        const dim3 grid(std::min(ntiles, per_cu * dev_ncu())), blk(256);
#define ROWDFT_CHAN4(K) LV(act_in ? "k_rowdft_chan4<" #K ">(act_in)" : "k_rowdft_chan4<" #K ">", rb, ntiles), launch("k_rowdft_chan4", k_rowdft_chan4<K>, grid, blk, lds, st, x, (float2*)x1, tfwd, C, g.P, g.W, g.Klast, rb, ntiles, act_in, 16 * g.NJ)
        if (K2P == 8) return ROWDFT_CHAN4(8);
        if (K2P == 16) return ROWDFT_CHAN4(16);
        return ROWDFT_CHAN4(32);
#undef ROWDFT_CHAN4
      }
    }
    // lanes <-> channels, persistent workgroups with a register-prefetched tile of CG channels x rb rows
    const int cg = 64, sl = 5;                      // one group of <= 64 channels, runs of <= 320 floats
    if (C <= 64 && g.W <= sl * 64) {
      int rb = std::max(1, std::min(std::min(chan_rb, g.P), sl * 64 / g.W));
      rb = std::max(1, std::min(rb, (int)((80 * 1024 / 4 / C - 1) / g.W)));
      while (rb > 1 && (long)B * ((g.P + rb - 1) / rb) < 4L * dev_ncu()) rb >>= 1;
      const size_t lds = (size_t)C * (rb * g.W + 1) * 4;
      const int ntiles = B * ((g.P + rb - 1) / rb);
      const int per_cu = std::max(1, (int)std::min<size_t>(4, FNO_LDS_MAX / lds));
      const dim3 grid(std::min(ntiles, per_cu * dev_ncu())), blk(256);
      (void)cg;
#define ROWDFT_CHAN(K) LV(act_in ? "k_rowdft_chan<" #K ",16>(act_in)" : "k_rowdft_chan<" #K ",16>", rb, ntiles), launch("k_rowdft_chan", k_rowdft_chan<K, 16>, grid, blk, lds, st, x, (float2*)x1, tT, C, g.P, g.W, g.Klast, rb, ntiles, act_in)
      if (K2P == 8) return ROWDFT_CHAN(8);
      if (K2P == 16) return ROWDFT_CHAN(16);
      return ROWDFT_CHAN(32);
#undef ROWDFT_CHAN
    }
  }
  // rows per workgroup: as many as keep the tile + table under 64 KB (several workgroups per CU), at most 8
  const int k2e = (g.Klast + 1) & ~1;
  int rb = 8;
  while (rb > 1 && ((size_t)C * (rb * g.W + 1) + (size_t)g.W * 2 * k2e) * 4 > 64 * 1024) rb >>= 1;
  const size_t lds = ((size_t)C * (rb * g.W + 1) + (size_t)g.W * 2 * k2e) * 4;
  if (lds > FNO_LDS_MAX) return fail(FNO_EUNSUPPORTED, "row tile of %d channels x %d floats exceeds LDS", C, g.W);
  return LV("k_rowdft_generic", rb, B * ((g.P + rb - 1) / rb)), launch("k_rowdft_generic", k_rowdft_generic, dim3(B * ((g.P + rb - 1) / rb)), dim3(256), lds, st, x, (float2*)x1,
                tfwd, C, g.P, g.W, g.Klast, rb);
}
static int row_inverse(hipStream_t st, const Geom& g, const float* tinv, const float* tT, int K2P, int B, int C,
                       const float* z, const float* bias,
                       float* y) {
  const size_t lds = pw_fwd_lds_bytes(2, C, 128, g.W, g.Klast, g.NJ, true, false);
  if (row_fast_ok(g, C) && lds <= 64 * 1024) {
    PwFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.z = z; a.tinv = tinv; a.bias = bias; a.u = y;
    a.PW = g.PW; a.W = g.W; a.P = g.P; a.K2in = g.Klast; a.K2out = 0; a.NJ = g.NJ;
    a.tiles_per_plane = g.PW / 128; a.ntiles = B * a.tiles_per_plane;
    const int grid = std::min(a.ntiles, 2 * dev_ncu());
    if (C == 32) return LV("k_pw_fwd<2,32,128>", 0, a.ntiles), launch("k_rowidft_tile", k_pw_fwd<2, 32, 128>, dim3(grid), dim3(256), lds, st, a);
    return LV("k_pw_fwd<2,64,128>", 0, a.ntiles), launch("k_rowidft_tile", k_pw_fwd<2, 64, 128>, dim3(grid), dim3(512), lds, st, a);
  }
  constexpr int chan_rb = 4;
  if (K2P) {
    // rows per workgroup: runs of <= 320 floats per channel, tile <= 78 KB (two workgroups per CU), >= 4 tiles per CU
    int rb = std::max(1, std::min(chan_rb, 320 / g.W));
    while (rb > 1 && ((size_t)C * (rb * g.W + 1) * 4 > 78 * 1024 || (long)B * ((g.P + rb - 1) / rb) < 4L * dev_ncu())) rb >>= 1;
    const size_t lds2 = (size_t)C * (rb * g.W + 1) * 4;
    if (C % 32 == 0 && g.W >= 32 && g.W <= 128) {   // truncated inverse DFT on the fp32 matrix cores (short rows would waste the 32-column tiles)
      const size_t tabb = (size_t)2 * g.Klast * (((g.W + 31) / 32) * 32 + 4) * 4;
      const size_t ldsf = (size_t)C * (ROWFLAT_CH + 4) * 4 + tabb;
      if (g.PW % 4 == 0 && g.W < ROWFLAT_CH && ldsf <= FNO_LDS_MAX && B <= 65535) {     // whole-line tiles of the flattened planes
        const dim3 gridf((g.PW + ROWFLAT_CH - 1) / ROWFLAT_CH, B);
        constexpr int flat_threads = 512;
        if (K2P == 8) return LV("k_rowidft_flat_mfma<8>", 0, (int)(gridf.x * gridf.y)), launch("k_rowidft_chan", k_rowidft_flat_mfma<8>, gridf, dim3(flat_threads), ldsf, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast);
        if (K2P == 16) return LV("k_rowidft_flat_mfma<16>", 0, (int)(gridf.x * gridf.y)), launch("k_rowidft_chan", k_rowidft_flat_mfma<16>, gridf, dim3(flat_threads), ldsf, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast);
        return LV("k_rowidft_flat_mfma<32>", 0, (int)(gridf.x * gridf.y)), launch("k_rowidft_chan", k_rowidft_flat_mfma<32>, gridf, dim3(flat_threads), ldsf, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast);
      }
      int rbm = rb;
      while (rbm > 1 && (size_t)C * (rbm * g.W + 1) * 4 + tabb > 80 * 1024) rbm >>= 1;
      const size_t lds3 = (size_t)C * (rbm * g.W + 1) * 4 + tabb;
      const dim3 gridm(B * ((g.P + rbm - 1) / rbm));
      if (lds3 <= FNO_LDS_MAX) {
        if (K2P == 8) return LV("k_rowidft_chan_mfma<8>", rbm, (int)gridm.x), launch("k_rowidft_chan", k_rowidft_chan_mfma<8>, gridm, dim3(256), lds3, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast, rbm);
        if (K2P == 16) return LV("k_rowidft_chan_mfma<16>", rbm, (int)gridm.x), launch("k_rowidft_chan", k_rowidft_chan_mfma<16>, gridm, dim3(256), lds3, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast, rbm);
        return LV("k_rowidft_chan_mfma<32>", rbm, (int)gridm.x), launch("k_rowidft_chan", k_rowidft_chan_mfma<32>, gridm, dim3(256), lds3, st, (const float2*)z, y, tinv, bias, C, g.P, g.W, g.Klast, rbm);
      }
    }
    if (lds2 <= FNO_LDS_MAX) {
      const dim3 grid(B * ((g.P + rb - 1) / rb));
      const dim3 blk(std::min(256, ((rb * C + 63) / 64) * 64));
      if (K2P == 8) return LV("k_rowidft_chan<8>", rb, (int)grid.x), launch("k_rowidft_chan", k_rowidft_chan<8>, grid, blk, lds2, st, (const float2*)z, y, tT, bias, C, g.P, g.W, g.Klast, rb);
      if (K2P == 16) return LV("k_rowidft_chan<16>", rb, (int)grid.x), launch("k_rowidft_chan", k_rowidft_chan<16>, grid, blk, lds2, st, (const float2*)z, y, tT, bias, C, g.P, g.W, g.Klast, rb);
      return LV("k_rowidft_chan<32>", rb, (int)grid.x), launch("k_rowidft_chan", k_rowidft_chan<32>, grid, blk, lds2, st, (const float2*)z, y, tT, bias, C, g.P, g.W, g.Klast, rb);
    }
  }
  int rb = 8;
  auto need = [&](int r) { return (((size_t)2 * g.Klast * g.W + 1) & ~(size_t)1) * 4 + (size_t)r * g.Klast * C * 8; };
  while (rb > 1 && need(rb) > 64 * 1024) rb >>= 1;
  if (need(rb) > FNO_LDS_MAX) return fail(FNO_EUNSUPPORTED, "row spectra of %d channels x %d bins exceed LDS", C, g.Klast);
  const dim3 grid(B * ((g.P + rb - 1) / rb));
  // (<= 32 kept bins always fit one of the tile / lanes-as-channels kernels above: plan creation refuses rows whose channel tile
  // exceeds LDS; what is left for the generic kernel is more than 32 bins, its run-time-bound form)
  return LV("k_rowidft_generic<0>", rb, (int)grid.x), launch("k_rowidft_generic", k_rowidft_generic<0>, grid, dim3(256), need(rb), st, (const float2*)z, y, tinv, bias, C,
                g.P, g.W, g.Klast, rb);
}

extern "C" int fno_spec_forward(const FnoSpecPlan* p, int B, const float* x, const float* const* wc, const float* bias,
                                float* y, float* xhat_save, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !x || !wc || !y || B < 1) return fail(FNO_EINVAL, "fno_spec_forward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (p->g.ndim == 1) return spec1d_forward(p, st, B, x, wc[0], bias, y, xhat_save, ws, ws_bytes);
  const Geom& g = p->g;
  const int Cin = p->d.Cin, Cout = p->d.Cout;
  bool ok;
  SpecWs w = carve_spec(p, B, ws, ws_bytes, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  float* hat = xhat_save ? xhat_save : w.hat_in;
  LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, Cin, x, w.x1, p->d.input_gelu));
  LAUNCHCHK(lead_forward(st, g, p->t, false, B, Cin, w.x1, w.tmp, hat));
  LAUNCHCHK(pack_w(st, g, Cin, Cout, wc, w.wp, xhat_save ? xhat_save + spec_xhat_floats(p, B) : w.wpt));
  LAUNCHCHK(mode_gemm(st, hat, w.wp, w.hat_out, B, g.Ktot, Cin, Cout, 0));
  LAUNCHCHK(lead_inverse(st, g, p->t, B, Cout, w.hat_out, w.tmp, w.z));
  LAUNCHCHK(row_inverse(st, g, p->t.tinv_f, p->t.tT[2], p->t.K2P, B, Cout, w.z, bias, y));
  return FNO_OK;
}

extern "C" int fno_spec_backward(const FnoSpecPlan* p, int B, const float* dy, const float* xhat, const float* const* wc,
                                 float* dx, float* const* dwc, float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !dy || B < 1) return fail(FNO_EINVAL, "fno_spec_backward: bad argument");
  if (dwc && !xhat) return fail(FNO_EINVAL, "weight gradients need the saved spectrum");
  if (dx && !wc && !xhat) return fail(FNO_EINVAL, "input gradient needs the weights (or the buffer saved by the forward)");
  hipStream_t st = (hipStream_t)stream;
  if (p->g.ndim == 1)
    return spec1d_backward(p, st, B, dy, xhat, wc ? wc[0] : nullptr, dx, dwc ? dwc[0] : nullptr, dbias, ws, ws_bytes);
  const Geom& g = p->g;
  const int Cin = p->d.Cin, Cout = p->d.Cout;
  bool ok;
  SpecWs w = carve_spec(p, B, ws, ws_bytes, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  if (dbias) {
    LAUNCHCHK(launch("k_channel_sums", k_channel_sums, dim3(64, Cout), dim3(256), 0, st, dy, w.dbpart, B, Cout, g.PW));
    LAUNCHCHK(reduce_slabs(st, w.dbpart, dbias, 64, 1, Cout, Cout, Cout));
  }
  if (!dx && !dwc) return FNO_OK;
  LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, Cout, dy, w.x1));
  LAUNCHCHK(lead_forward(st, g, p->t, true, B, Cout, w.x1, w.tmp, w.hat_out));   // G
  if (dwc) {
    LAUNCHCHK(mode_gemm_dw(st, xhat, w.hat_out, w.dwp, B, g.Ktot, Cin, Cout));
    LAUNCHCHK(unpack_dw(st, g, Cin, Cout, w.dwp, dwc));
  }
  if (dx) {
    const float* wpt = xhat ? xhat + spec_xhat_floats(p, B) : w.wpt;                 // packed by the forward when it saved
    if (!xhat) LAUNCHCHK(pack_w(st, g, Cin, Cout, wc, w.wp, w.wpt));
    LAUNCHCHK(mode_gemm(st, w.hat_out, wpt, w.hat_in, B, g.Ktot, Cout, Cin, 1));     // GX
    LAUNCHCHK(lead_inverse(st, g, p->t, B, Cin, w.hat_in, w.tmp, w.z));
    LAUNCHCHK(row_inverse(st, g, p->t.tinv_b, p->t.tT[3], p->t.K2P, B, Cin, w.z, nullptr, dx));
  }
  return FNO_OK;
}

// ==========================================================================
// fused FNO model
// ==========================================================================
struct FnoModelPlan {
  FnoModelDesc d;
  Geom g;
  Tables t;
  int NPX;      // pixels per workgroup tile (128 or 256)
  bool loose;   // rows do not tile the pixel tile (last dim 96, 160, 73, ...): spectral rows gathered per tile, separate row-DFT passes
  int ncu;      // compute units of the device the plan was made on
  // What a forward pass left in ITS `saved` buffer - the backward pass that reads the buffer must take the matching paths.
  // Plans are cached and shared by every call with the same configuration (other batch sizes, other models, other threads),
  // so this lives per `saved` buffer, not per plan: forward records it under the buffer's address, backward looks it up (a
  // buffer the plan has never seen reads as "nothing published": the three-term paths, which need no bounds).
  struct CallState {
    bool u0_skipped = false;     // u_0 (the lifting output) was not written: block 0 recomputes it
    bool h2_fwd = false;         // max |u_L| was published behind the saved tensors (two-term fp16 projection / block backward)
    bool h2_u0 = false;          // ... and the bound of |u_0| (fused lifting)
    bool gchain_valid = false;   // the last backward part left max |g| of its output gradient (amax[32 + l_lo])
    bool bwd_clean = false;      // the forward cleared all bound slots and no backward pass has written its range [32, 64) since
    int B = 0;                   // batch of the forward that published this record (a relocated copy of another
                                 // forward's `saved` can land on this address - a record for a different batch is a miss)
  };
  mutable std::mutex call_mu;
  mutable std::vector<std::pair<const void*, CallState>> calls;      // most recent last; capped (kMaxCalls)
  static const size_t kMaxCalls = 4096;
  void put_call(const void* saved, const CallState& cs) const {
    std::lock_guard<std::mutex> lk(call_mu);
    for (size_t i = 0; i < calls.size(); ++i)
      if (calls[i].first == saved) { calls.erase(calls.begin() + i); break; }
    if (calls.size() >= kMaxCalls) calls.erase(calls.begin());
    calls.emplace_back(saved, cs);
  }
  // miss (`found` = false): the buffer was evicted (more than kMaxCalls forwards since) or autograd handed `saved` back at another
  // address (saved_tensors_hooks, offload, checkpoint repack).  The caller then falls back to what a forward pass of this plan
  // does under the current switches for u0_skipped (model_backward_impl) and to the three-term paths, which need no bounds.
  CallState get_call(const void* saved, int B, bool* found) const {
    std::lock_guard<std::mutex> lk(call_mu);
    for (size_t i = calls.size(); i-- > 0;)
      if (calls[i].first == saved) {
        if (calls[i].second.B != B) break;      // stale: another forward's record for this address
        *found = true;
        return calls[i].second;
      }
    *found = false;
    return CallState();
  }
};

static const int kHID = 256;
// Magnitude bounds kept at the end of the forward's `saved` buffer (fno_dev.h "h2"): kNAmax floats, the slots not named here
// stay 0.  tests/test_hostile_ranges_gpu.py checks every slot by its NUMBER - the independent statement of this map.
static const int kNAmax = 64;
static const int kBndX = 7;                                    // max |x| of the model input (k_lift_rowdft)
// max |u_l| as stored (l >= 1); l = 0: the bound of |u_0| block 0's forward derives from max |x| (fused lifting: lift_u0_bound)
static constexpr int bnd_u(int l) { return 8 + l; }
static constexpr int bnd_g(int l) { return 32 + l; }           // max |dL/du_l| (the backward's gradient chain, l >= 1)
// the projection backward's scalars: max |dy|, max |W1|, max |w2| (the kernels read them as amax[1..3] behind kBndProj)
static const int kBndProj = 59, kBndDy = kBndProj + 1, kBndW1 = kBndProj + 2, kBndW2 = kBndProj + 3;
static_assert(kBndX < bnd_u(0) && bnd_u(FNO_MAX_LAYERS) < bnd_g(0) && bnd_g(FNO_MAX_LAYERS) < kBndProj && kBndW2 < kNAmax,
              "bound slots: [8, 32) forward |u_l|, [32, 59) backward |g_l|, [59, 63) projection scalars");
// persistent-grid size per CU of the forward kernels (= workgroups that fit: registers / LDS)
static constexpr int FNO_GRID_LIFT = 3;
static constexpr int FNO_GRID_PW = 2;
static constexpr int FNO_GRID_BWD = 1;   // persistent workgroups per CU of the backward kernels: their LDS footprint allows one resident
                                         // workgroup, and every extra one adds a partial slab to reduce
static constexpr int FNO_GRID_PWX = 4;
static constexpr int FNO_NTW_PWX = 2;    // 4-wave workgroups, two per CU
static constexpr int FNO_GRID_PF = 1;

extern "C" int fno_model_plan_create(const FnoModelDesc* d, FnoModelPlan** out) {
  if (!d || !out) return fail(FNO_EINVAL, "null argument");
  if (d->n_layers < 1 || d->n_layers > FNO_MAX_LAYERS) return fail(FNO_EINVAL, "n_layers=%d", d->n_layers);
  if (d->C != 32 && d->C != 64) return fail(FNO_EUNSUPPORTED, "fused path supports hidden width 32 or 64 (got %d)", d->C);
  // Cin == 0: no lifting (x is the (B, C, ...) input of block 0); Cout == 0: no projection (y = u_L)
  if (d->Cin < 0 || d->Cin > 4) return fail(FNO_EUNSUPPORTED, "fused path supports 0..4 input channels (got %d)", d->Cin);
  if (d->Cout < 0 || d->Cout > PROJ_MAXCO) return fail(FNO_EUNSUPPORTED, "fused path supports 0..%d output channels", PROJ_MAXCO);
  if (d->Cout > 0 && d->hidden_proj != kHID)
    return fail(FNO_EUNSUPPORTED, "fused path supports projection_channels=256 (got %d)", d->hidden_proj);
  if (d->Cout == 0 && ((d->gelu_mask >> (d->n_layers - 1)) & 1u))
    return fail(FNO_EUNSUPPORTED, "a block stack without projection must end without activation");
  FnoModelPlan* p = new FnoModelPlan();
  p->d = *d;
  int rc = make_geom(p->g, d->ndim, d->dims, d->modes, 0, d->norm, d->weight_planes);
  if (rc == FNO_OK) {
    const int W = p->g.W;
    p->loose = false;
    const int npx_tiled = W > 128 ? 256 : 128;
    const bool tiles = W % 32 == 0 && W <= 256 && npx_tiled % W == 0 && p->g.PW % npx_tiled == 0;
    if (!tiles && W >= 32 && W <= 320 && p->g.PW % 128 == 0 && p->g.Klast <= 32) {
      // "loose rows" (the PINO observers' padded time axis, 73; FNO grids such as 96 x 96 or 160 x 160): 128-pixel tiles of
      // the flattened plane; the block kernels take the spectral rows that overlap their tile (kext_loose_rows) and the
      // last-dim forward transforms
      // run as separate lanes-as-channels passes instead of kernel epilogues.  Block stacks only.
      p->loose = true;
      p->NPX = 128;
    } else if (W % 32 != 0 || W > 256) rc = fail(FNO_EUNSUPPORTED, "fused path needs last dim %% 32 == 0 and <= 256 (got %d)", W);
    else {
      p->NPX = W > 128 ? 256 : 128;
      if (p->NPX % W != 0 || p->g.PW % p->NPX != 0)
        rc = fail(FNO_EUNSUPPORTED, "plane of %d pixels (W=%d) does not tile by %d", p->g.PW, W, p->NPX);
    }
    if (rc == FNO_OK && p->g.NJ > 4) rc = fail(FNO_EUNSUPPORTED, "too many last-dim modes (%d)", p->g.Klast);
    if (rc == FNO_OK) {
      // every kernel of the plan must fit its tile + twiddle tables in FNO_LDS_MAX (256-pixel tiles with many kept last-dim
      // modes do not: such shapes take the unfused composition).  The sums below approximate blk_bwd_lds_bytes,
      // blk_bwd_t_lds_bytes (and its loose form), pw_fwd_x3_lds_bytes and pw_fwd_lds_bytes of the kernel headers; they are kept
      // as they are because which plans are accepted is ABI behaviour.
      const Geom& g = p->g;
      const int npx = p->NPX, C = d->C;
      const size_t tz = ((size_t)2 * g.Klast * g.W + (size_t)(npx / g.W + (p->loose ? 2 : 0)) * g.Klast * C * 2) * 4;   // inverse table + Z rows
      const size_t tf = (size_t)16 * g.NJ * (g.W + 4) * 4;                                          // forward table
      const bool many = d->n_layers > 1 && !p->loose;      // blocks above 0 also carry the forward table
      const size_t xin = d->Cin > 0 ? (size_t)8 * (npx + 4) * 4 : 0;                                // block 0: lifting rows
      const size_t bbwd_f32 = (size_t)2 * C * (npx + 4) * 4 + tz + std::max(xin, many ? tf : (size_t)0);
      const size_t bbwd_x3 = (size_t)6 * C * (npx + 8) * 2 + (size_t)C * (npx + 4) * 4 + tz + std::max(xin, many ? tf : (size_t)0);
      const size_t bbwd = (npx == 128 && bbwd_x3 <= FNO_LDS_MAX) ? bbwd_x3 : bbwd_f32;
      const size_t pwx3 = (size_t)3 * npx * (C + 8) * 2 + tz + (many ? tf : 0), pwf32 = (size_t)C * (npx + 4) * 4 + tz + (many ? tf : 0);
      // loose rows exist for the split-precision kernels only; their backward kernel can apply the K-extension in chunks
      // of kept modes, so one mode's rows + table column must fit next to the GEMM images
      const size_t bbwd_x3_1 = (size_t)6 * C * (npx + 8) * 2 + (size_t)C * (npx + 4) * 4 +
                               ((size_t)2 * g.W + (size_t)(npx / g.W + 2) * C * 2) * 4;
      if (p->loose && (bbwd_x3_1 > FNO_LDS_MAX || pwx3 > FNO_LDS_MAX))
        rc = fail(FNO_EUNSUPPORTED, "loose-row tile of %d channels with %d kept last-dim modes exceeds LDS", C, g.Klast);
      else if (p->loose) { /* fits */ }
      else if (bbwd > FNO_LDS_MAX || pwx3 > FNO_LDS_MAX || pwf32 > FNO_LDS_MAX)
        rc = fail(FNO_EUNSUPPORTED, "tile of %d pixels x %d channels with %d kept last-dim modes exceeds LDS", npx, C,
                  g.Klast);
    }
  }
  if (rc == FNO_OK) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
      rc = fail(FNO_EHIP, "no HIP device");
    else p->ncu = prop.multiProcessorCount;
  }
  if (rc == FNO_OK) rc = make_tables(p->g, p->t);
  if (rc != FNO_OK) { p->t.release(); delete p; return rc; }
  *out = p;
  return FNO_OK;
}
extern "C" void fno_model_plan_destroy(FnoModelPlan* p) {
  if (!p) return;
  p->t.release();
  delete p;
}

struct ModelSizes {
  size_t n_act, n_x1, n_tmp, n_hat, n_wp;
  int grid_bb;      // workgroups of the block-backward launches (its partial slabs are sized by it)
  int ntiles, tiles_per_plane, grid;
};
static ModelSizes model_sizes(const FnoModelPlan* p, int B) {
  const Geom& g = p->g;
  const int C = p->d.C;
  ModelSizes s;
  s.n_act = (size_t)B * C * g.PW;
  s.n_x1 = (size_t)B * g.P * g.Klast * C * 2;
  s.n_tmp = g.nlead == 2 ? (size_t)B * g.dims[0] * g.Klead[1] * g.Klast * C * 2 : 1;
  s.n_hat = (size_t)B * g.Ktot * C * 2;
  s.n_wp = (size_t)g.Ktot * C * C * 2;
  s.tiles_per_plane = g.PW / p->NPX;
  s.ntiles = B * s.tiles_per_plane;
  s.grid = std::min(s.ntiles, FNO_GRID_BWD * p->ncu);
  // block backward at 32 channels: 4-wave workgroups of ~75 KB LDS, two fit a CU (k_block_bwd_t)
  s.grid_bb = (p->d.C == 32 && g_gemm_x3 && p->NPX == 128) ? std::min(s.ntiles, 2 * p->ncu) : s.grid;
  return s;
}

struct ModelWs {
  float *x1, *tmp, *hat, *ohat, *z, *wp, *wpt, *w1p;
  unsigned short *wa1, *wa3;
  // backward only
  float *ga, *gb, *dwp, *dw_part, *db_part, *dwl_part, *dw1_part, *db1_part, *dw2_part, *db2_part;
  size_t total;
};
static ModelWs carve_model(const FnoModelPlan* p, int B, void* ws, size_t cap, bool backward, bool* ok) {
  const ModelSizes s = model_sizes(p, B);
  const int C = p->d.C;
  Carver c(ws, cap);
  ModelWs w;
  memset(&w, 0, sizeof(w));
  w.x1 = c.take<float>(s.n_x1);
  w.tmp = c.take<float>(s.n_tmp);
  w.hat = c.take<float>(s.n_hat);
  w.ohat = c.take<float>((size_t)p->d.n_layers * s.n_hat);   // the gradient spectrum of EVERY layer (one batched weight-gradient contraction)
  w.z = c.take<float>(s.n_x1);
  w.wp = c.take<float>(s.n_wp);
  w.wpt = c.take<float>(s.n_wp);
  w.w1p = c.take<float>((size_t)kHID * C);
  w.wa1 = c.take<unsigned short>((size_t)(kHID / 32) * (C / 16) * 3 * 64 * 8);
  w.wa3 = c.take<unsigned short>((size_t)(kHID / 32) * 2 * (C / 32) * 3 * 64 * 8);
  if (backward) {
    w.ga = c.take<float>(s.n_act);
    w.gb = c.take<float>(s.n_act);
    w.dwp = c.take<float>((size_t)p->d.n_layers * s.n_wp);
    w.dw_part = c.take<float>((size_t)p->d.n_layers * s.grid_bb * ((p->NPX / 32) / (C / 32)) * C * C);
    w.db_part = c.take<float>((size_t)p->d.n_layers * s.grid_bb * C);
    w.dwl_part = c.take<float>((size_t)s.grid_bb * C * 16);
    w.dw1_part = c.take<float>((size_t)s.grid * kHID * C);
    w.db1_part = c.take<float>((size_t)s.grid * 8 * kHID);
    w.dw2_part = c.take<float>((size_t)s.grid * 8 * PROJ_MAXCO * kHID);
    w.db2_part = c.take<float>((size_t)64 * PROJ_MAXCO);
  }
  w.total = c.off;
  if (ok) *ok = c.ok;
  return w;
}
extern "C" size_t fno_model_workspace_bytes(const FnoModelPlan* p, int B) {
  return carve_model(p, B, nullptr, 0, true, nullptr).total;
}
// the forward's `saved` buffer: u_0 .. u_L, every layer's truncated input spectrum and packed weights (kept for backward), the
// magnitude bounds
// (u[l] = u + l * n_act, hats[l] = hats + l * n_hat; wps [k][i][o] and wpts, the transposed copy [k][o][i]: n_wp floats per layer)
struct ModelSaved { float *u, *hats, *wps, *wpts, *bounds; size_t total; };
static ModelSaved carve_saved(const FnoModelPlan* p, int B, const void* saved) {
  const ModelSizes s = model_sizes(p, B);
  const size_t nl = p->d.n_layers;
  float* base = (float*)const_cast<void*>(saved);
  size_t off = 0;
  auto take = [&](size_t n) { float* q = base ? base + off : nullptr; off += n; return q; };
  ModelSaved v;
  v.u = take((nl + 1) * s.n_act);
  v.hats = take(nl * s.n_hat);
  v.wps = take(nl * s.n_wp);
  v.wpts = take(nl * s.n_wp);
  v.bounds = take(kNAmax);
  v.total = off * sizeof(float);
  return v;
}
extern "C" size_t fno_model_saved_bytes(const FnoModelPlan* p, int B) { return carve_saved(p, B, nullptr).total; }
// the tile geometry PwFwdArgs and BlkBwdArgs carry
template <typename A>
static void set_tile_geom(A& a, const Geom& g, const ModelSizes& s, int K2in) {
  a.PW = g.PW; a.W = g.W; a.P = g.P; a.K2in = K2in; a.K2out = g.Klast; a.NJ = g.NJ;
  a.tiles_per_plane = s.tiles_per_plane; a.ntiles = s.ntiles;
}
// corner tensors of layers lo .. hi -> slots 0 .. hi - lo of the pack / unpack kernels' pointer table
template <typename CP, typename P>
static CP corner_ptrs(const Geom& g, P spec_w, int lo, int hi) {
  CP cp;
  memset(&cp, 0, sizeof(cp));
  for (int l = lo; l <= hi; ++l)
    for (int c = 0; c < (1 << g.nlead); ++c) cp.p[l - lo][c] = (std::remove_reference_t<decltype(cp.p[0][0])>)spec_w[l][c];
  return cp;
}

// ---- templated launch dispatch ---------------------------------------------
template <int CIN, int COUT>
static int launch_pw(const FnoModelPlan* p, hipStream_t st, int grid, const PwFwdArgs& a, const char* name) {
  const size_t lds = pw_fwd_lds_bytes(CIN, COUT, p->NPX, a.W, a.K2in, a.NJ, a.z != nullptr, a.x1 != nullptr);
  if (p->NPX == 128)
    return GT(1), launch(name, k_pw_fwd<CIN, COUT, 128>, dim3(grid), dim3((COUT / 32) * 4 * 64), lds, st, a);
  return GT(1), launch(name, k_pw_fwd<CIN, COUT, 256>, dim3(grid), dim3((COUT / 32) * 8 * 64), lds, st, a);
}
static int launch_lift(const FnoModelPlan* p, hipStream_t st, int grid, const PwFwdArgs& a) {
  const int C = p->d.C;
  switch (p->d.Cin * 100 + C) {
    case 132: return launch_pw<1, 32>(p, st, grid, a, "k_pw_fwd_lift");
    case 232: return launch_pw<2, 32>(p, st, grid, a, "k_pw_fwd_lift");
    case 332: return launch_pw<3, 32>(p, st, grid, a, "k_pw_fwd_lift");
    case 432: return launch_pw<4, 32>(p, st, grid, a, "k_pw_fwd_lift");
    case 164: return launch_pw<1, 64>(p, st, grid, a, "k_pw_fwd_lift");
    case 264: return launch_pw<2, 64>(p, st, grid, a, "k_pw_fwd_lift");
    case 364: return launch_pw<3, 64>(p, st, grid, a, "k_pw_fwd_lift");
    case 464: return launch_pw<4, 64>(p, st, grid, a, "k_pw_fwd_lift");
  }
  return fail(FNO_EUNSUPPORTED, "lifting %d -> %d", p->d.Cin, C);
}
// block 0 of a model with a lifting layer computes u_0 = W_l x + b_l itself (forward on load, backward from the input rows it
// stages anyway) when both of its kernels are the split-precision 128-pixel ones: u_0 then never travels through HBM
static bool lift_fused(const FnoModelPlan* p) {
  return p->d.Cin > 0 && g_gemm_x3 && p->NPX == 128 && !p->loose;
}
// second-generation block forward (k_block_fwd2.h): whole rows in 128-pixel tiles, two workgroups per CU
template <int C>
static bool blk_fwd_t_ok(const FnoModelPlan* p, const PwFwdArgs& a, size_t* lds) {
  if (p->NPX != 128 || p->loose || !a.x) return false;
  if ((size_t)a.PW * 4 * C >= (size_t)1 << 31) return false;          // 32-bit buffer offsets within one sample
  if (a.z && a.K2in > 8) return false;      // more than 8 kept last-dim modes (two extension k blocks, e.g. RNO2d at 12): k_pw_fwd_x3
                                            // is as fast or faster (RNO2d 128^2: 0.085 vs 0.108 ms per launch)
  if (C == 32) return false;      // 32 channels: k_pw_fwd_x3 is faster with and without a row-DFT epilogue (FNO3d 64^3: 0.298 vs 0.329 ms per launch,
                                  // BASELINE config 1: 11.2 vs 11.7 us)
  *lds = blk_fwd_t_lds_bytes(C, a.W, a.K2in, a.NJ, a.z != nullptr, a.x1 != nullptr);
  return *lds + 2048 <= FNO_LDS_MAX;
}
// third-generation block forward (k_block_fwd3.h): independent strip waves fed by LDS-DMA.  64 channels, rows of 128 pixels,
// <= 8 kept last-dim modes either side, two-term fp16 mode, no lifting / ReLU / addend; everything else keeps k_blk_fwd_t.
// u is bit-identical to k_blk_fwd_t's (same products in the same order), x1 agrees to ~2e-7 (fp16-split row DFT instead of
// fp32 MFMAs).  FNO_BFWD_V2=1 keeps the second generation (A/B arm).
static const int g_bfwd_v2 = getenv("FNO_BFWD_V2") ? 1 : 0;
static const int g_zigzag = getenv("FNO_NO_ZIGZAG") ? 0 : 1;      // A/B switch: alternating tile order along the kernel chain
static bool blk_fwd_s_ok(const FnoModelPlan* p, const PwFwdArgs& a, size_t* lds) {
  if (g_bfwd_v2 || p->NPX != 128 || p->loose || !a.x || !a.u || !a.z || !a.xmax) return false;
  if (a.W != 128 || a.K2in < 1 || a.K2in > 8 || a.relu_out || a.add || (a.lw && a.CL > 4)) return false;
  if (a.x1 && (a.NJ != 1 || a.K2out > 8)) return false;
  if ((size_t)a.PW * 4 * 64 >= (size_t)1 << 31) return false;          // 32-bit offsets within one sample
  *lds = blk_fwd_s_lds_bytes(a.K2out, a.x1 != nullptr);
  return *lds <= FNO_LDS_MAX;      // (uniformity only: at most 82 KB with K2out <= 8)
}
// k_blk_fwd_s has every ACT_IN x EPI combination without lifting and every EPI with it (nine instantiations)
template <bool ACT_IN, bool LIFT>
static int launch_blk_fwd_s(const char* nm, hipStream_t st, dim3 grid, size_t lds, int epi, const PwFwdArgs& a) {
  if (epi == 2) return launch(nm, k_blk_fwd_s<ACT_IN, 2, LIFT>, grid, dim3(256), lds, st, a);
  if (epi == 1) return launch(nm, k_blk_fwd_s<ACT_IN, 1, LIFT>, grid, dim3(256), lds, st, a);
  return launch(nm, k_blk_fwd_s<ACT_IN, 0, LIFT>, grid, dim3(256), lds, st, a);
}
// A block's forward in the split mode.  In this order:
//   k_blk_fwd_s   two fp16 terms     where k_blk_fwd_t is eligible AND blk_fwd_s_ok (the bound of |x| is known, ...)
//   k_blk_fwd_t   three bf16 terms   64 channels, whole rows in 128-pixel tiles (blk_fwd_t_ok), the listed flag combinations
//   k_pw_fwd_x3   three bf16 terms   everything else (every option is a run-time argument)
// *ub_published (if given): the launched kernel left the bound of |u_0| at a.ubound.  The LIFT variant of each family does when
// a.xmax is set (lift_u0_bound, fno_dev.h) - the two-term block-0 backward splits u_0 by it, so the host hands it on only when it
// was written.
template <int C>
static int launch_block_x3(const FnoModelPlan* p, hipStream_t st, int grid, const PwFwdArgs& a, bool* ub_published = nullptr) {
  bool unused = false;
  bool& published = ub_published ? *ub_published : unused;
  published = false;
  const bool lift_ub = a.lw && a.ubound && a.xmax;      // what a LIFT variant publishes
  // profile label: block 0 with the lifting recomputed reads the <= 4-channel model input instead of u_0 (bench.py prices it so)
  const char* nm = a.lw ? "k_pw_fwd_block0" : "k_pw_fwd_block";
  // (64 channels only: blk_fwd_t_ok refuses 32, where k_pw_fwd_x3 measured faster - `if constexpr` so that the 33 instantiations
  // nothing can launch are not compiled: tools/kernel_coverage.py, round 5)
  size_t lds_t = 0, lds_s = 0;
  if constexpr (C == 64) if (blk_fwd_t_ok<C>(p, a, &lds_t)) {
    const dim3 g2(std::min(a.ntiles, 2 * p->ncu)), blk((C / 32) * 2 * 64);
    const int epi = a.x1 ? (a.act_out ? 2 : 1) : 0;
    // two workgroups per CU: the one dispatched first gets the larger share of the CU's tiles (pair_share, fno_dev.h)
    constexpr int share_bf = 20;      // of 32 (16 = even): 2.111 / 2.114 / 2.103 / 2.110 ms per step at 18 / 16 / 20 / 22 (round 6, one box)
    PwFwdArgs at = a;
    at.share32 = ((int)g2.x == 2 * p->ncu) ? share_bf : 0;
    if (blk_fwd_s_ok(p, a, &lds_s)) {      // the strip kernel: the model path's two-term combinations
      published = lift_ub;
      GT(2);
      if (a.lw) return launch_blk_fwd_s<false, true>(nm, st, g2, lds_s, epi, at);
      if (a.act_in) return launch_blk_fwd_s<true, false>(nm, st, g2, lds_s, epi, at);
      return launch_blk_fwd_s<false, false>(nm, st, g2, lds_s, epi, at);
    }
    // k_blk_fwd_t (three-term variants: its two-term ones were replaced by the strip kernel above) for the flag combinations the
    // models and layer stacks of the reference produce - every instantiation below is launched by the GPU test suite
    // (tools/kernel_coverage.py); anything else takes k_pw_fwd_x3.  Not a helper: the list does not enumerate every combination.
    // (template flags: LIFT, RELU, ACT_IN, EPI, ADD, KZ - k_block_fwd2.h)
#define BF2(LIFT_, RELU_, AIN_, EPI_, ADD_, KZ_) return GT(3), launch(nm, k_blk_fwd_t<C, LIFT_, RELU_, AIN_, EPI_, ADD_, KZ_>, g2, blk, lds_t, st, at)
    const int kz = a.z ? (2 * a.K2in + 15) / 16 : 0;
    const bool plain = !a.lw && !a.relu_out && !a.add;
    if (kz == 1) {
      if (a.lw && !a.relu_out && !a.add && epi == 2) { published = lift_ub; BF2(true, false, false, 2, false, 1); }
      if (plain && a.act_in) { if (epi == 2) BF2(false, false, true, 2, false, 1); if (epi == 1) BF2(false, false, true, 1, false, 1); BF2(false, false, true, 0, false, 1); }
      if (plain) { if (epi == 2) BF2(false, false, false, 2, false, 1); if (epi == 1) BF2(false, false, false, 1, false, 1); BF2(false, false, false, 0, false, 1); }
      if (!a.lw && a.relu_out && !a.add && epi == 0 && !a.act_in) BF2(false, true, false, 0, false, 1);
    } else if (kz == 0 && epi == 0 && !a.lw && !a.relu_out) {      // pointwise layers (no spectral branch), with or without an addend
      if (a.add) { if (a.act_in) BF2(false, false, true, 0, true, 0); BF2(false, false, false, 0, true, 0); }
      if (!a.act_in) BF2(false, false, false, 0, false, 0);
    }
#undef BF2
  }
  // k_pw_fwd_x3 (template flags behind the tile shape: LOOSE, LIFT, RELU); no fallback behind it: launch() refuses what exceeds LDS
  const size_t lds = pw_fwd_x3_lds_bytes(C, p->NPX, a.W, a.K2in, a.NJ, a.z != nullptr, a.x1 != nullptr) +
                     (p->loose && a.z ? (size_t)2 * a.K2in * C * 2 * 4 : 0);      // two more spectral rows per tile
  const dim3 blk((C / 32) * (4 / FNO_NTW_PWX) * 64);
#define PWX(...) return GT(3), launch(nm, k_pw_fwd_x3<C, 128, FNO_NTW_PWX, ##__VA_ARGS__>, dim3(grid), blk, lds, st, a)
  if (p->loose && !a.relu_out) PWX(true);
  if (a.lw && !a.relu_out) { published = lift_ub; PWX(false, true); }
  if (a.relu_out) {
    if (p->NPX != 128 || p->loose || a.lw) return fail(FNO_EUNSUPPORTED, "ReLU output: 128-pixel tiles of whole rows, no fused lifting");
    PWX(false, false, true);
  }
  if (p->NPX == 128) PWX();
#undef PWX
  return GT(3), launch(nm, k_pw_fwd_x3<C, 256, 2>, dim3(grid), dim3((C / 32) * 4 * 64), lds, st, a);
}
static int launch_block(const FnoModelPlan* p, hipStream_t st, int grid, const PwFwdArgs& a, bool* ub_published = nullptr) {
  if (ub_published) *ub_published = false;
  if (p->loose && !g_gemm_x3) return fail(FNO_EUNSUPPORTED, "block stacks on loose rows need the split-precision GEMM mode");
  if (g_gemm_x3) return p->d.C == 32 ? launch_block_x3<32>(p, st, grid, a, ub_published) : launch_block_x3<64>(p, st, grid, a, ub_published);
  if (a.relu_out) {      // one-layer stacks with a ReLU tail: the exact-fp32 twin of k_pw_fwd_x3<.., RELU = true>
    if (p->NPX != 128 || p->loose || a.lw) return fail(FNO_EUNSUPPORTED, "ReLU output: 128-pixel tiles of whole rows, no fused lifting");
    const size_t lds = pw_fwd_lds_bytes(p->d.C, p->d.C, 128, a.W, a.K2in, a.NJ, a.z != nullptr, a.x1 != nullptr);
    if (p->d.C == 32)
      return GT(1), launch("k_pw_fwd_block", k_pw_fwd<32, 32, 128, true>, dim3(grid), dim3(1 * 4 * 64), lds, st, a);
    return GT(1), launch("k_pw_fwd_block", k_pw_fwd<64, 64, 128, true>, dim3(grid), dim3(2 * 4 * 64), lds, st, a);
  }
  if (p->d.C == 32) return launch_pw<32, 32>(p, st, grid, a, "k_pw_fwd_block");
  return launch_pw<64, 64>(p, st, grid, a, "k_pw_fwd_block");
}
// k_block_bwd_g2 (k_block_bwd2.h; 64 channels, rows of 32 / 64 / 128 pixels: two independent 4-wave groups per workgroup): the
// shape conditions, the two variants the register budget allows - block 0 with the lifting recomputed, and a block without
// lifting input (gradient addends and two 16-output row-DFT blocks per wave: k_block_bwd_t takes those) - and the LDS check.
// Decides a.kx16 and a.lines, which only this kernel reads.
static bool blk_bwd_g2_ok(const FnoModelPlan* p, BlkBwdArgs& a, bool h2, size_t* lds) {
  const int nterm = h2 ? 2 : 3;
  // the K-extension as one 16-deep block on the matrix pipe where its images fit (judged before the whole-line staging is
  // added: kept as it was, the other order could change what runs)
  a.kx16 = (a.zg && a.K2in <= 8) ? 1 : 0;
  if (a.kx16 && blk_bwd_g2_lds_bytes(a, nterm) > FNO_LDS_MAX) a.kx16 = 0;
  a.lines = h2 ? 1 : 0;      // whole-line u loads / gout stores (round 6): the two-term variants carry them
  if (!g_gemm_x3 || p->NPX != 128 || (a.W != 32 && a.W != 64 && a.W != 128) || (a.x1g && a.NJ > 2) || a.ntiles < 2) return false;
  const bool two = a.x1g && a.W == 128 && a.NJ == 2;
  if (a.gadd || (a.lw ? a.x1g != nullptr : (a.xin || two))) return false;
  *lds = blk_bwd_g2_lds_bytes(a, nterm);
  return *lds <= FNO_LDS_MAX;
}
// A block's backward.  In this order:
//   spectral-branch dropout     k_block_bwd_t<DROPK> (three bf16 terms) / k_block_bwd<DROPK> (exact fp32)
//   loose rows                  k_block_bwd_t<LOOSE> (three bf16 terms), the K-extension in chunks that fit LDS
//   k_block_bwd_g2              64 channels (blk_bwd_g2_ok): two fp16 terms when both operand bounds came, else three bf16 terms
//   k_block_bwd_t               split mode, 128-pixel tiles: two fp16 terms at 32 channels when the bounds came, else three bf16
//   k_block_bwd                 exact fp32: everything else without a recomputed lifting
// *published (if given): the launched kernel left max |gout| at a.gmax_out (k_block_bwd_g2 and k_block_bwd_t outside the
// dropout / loose rows, when the pointer is set)
template <int C>
static int launch_bbwd_c(const FnoModelPlan* p, hipStream_t st, int grid, const BlkBwdArgs& a_in, bool* published_out = nullptr) {
  BlkBwdArgs a = a_in;
  bool unused = false;
  bool& published = published_out ? *published_out : unused;
  published = false;
  // profile labels: block 0 behind a lifting layer reads g and the model input and writes no gradient tile unless dx is asked for
  const char* nm = (a.xin && !a.gout) ? "k_block_bwd0" : "k_block_bwd";
  const bool h2 = a.gmax_in && a.umax;      // two-term fp16 variants (operand bounds known)
  const dim3 blk(BlkBwdCfg<C, 128>::NW * 64);
  const size_t lds_t = blk_bwd_t_lds_bytes(C, a);      // (in every mode: it divides by a.W only under a.zg, and W is set with zg)
  const bool t_ok = g_gemm_x3 && p->NPX == 128 && lds_t <= FNO_LDS_MAX;      // k_block_bwd_t
  if (a.drop_seed) {      // dropout of the spectral branch (one-layer stacks with a tail, fno_model_*_tail)
    const size_t lds_f = blk_bwd_lds_bytes(C, 128, a);
    if (p->loose || a.lw || a.xin || p->NPX != 128 || (g_gemm_x3 ? lds_t : lds_f) > FNO_LDS_MAX)
      return fail(FNO_EUNSUPPORTED, "spectral-branch dropout: 128-pixel tiles of whole rows, no lifting");
    if (!g_gemm_x3)      // exact-fp32 mode: the first-generation kernel with the same regenerated mask
      return GT(1), launch(nm, k_block_bwd<C, 128, true>, dim3(grid), blk, lds_f, st, a);
    return GT(3), launch(nm, k_block_bwd_t<C, 128, false, false, true>, dim3(grid), blk, lds_t, st, a);
  }
  if (p->loose) {
    if (!g_gemm_x3) return fail(FNO_EUNSUPPORTED, "block stacks on loose rows need the split-precision GEMM mode");
    int kch = a.K2in;
    while (kch > 1 && blk_bwd_t_loose_lds_bytes(C, a, kch) > FNO_LDS_MAX) --kch;         // chunk the K-extension until the tile fits
    const size_t lds_l = blk_bwd_t_loose_lds_bytes(C, a, kch);
    if (a.zg && lds_l > FNO_LDS_MAX) return fail(FNO_EUNSUPPORTED, "loose-row backward tile exceeds LDS");
    if (a.zg) a.kch = kch < a.K2in ? kch : 0;
    return GT(3), launch(a.kch ? "k_block_bwd_kch" : nm, k_block_bwd_t<C, 128, true>, dim3(grid), blk, lds_l, st, a);
  }
  if constexpr (C == 64) {
    size_t lds_g2 = 0;
    if (blk_bwd_g2_ok(p, a, h2, &lds_g2)) {
      published = a.gmax_out != nullptr;
      GT(h2 ? 2 : 3);
      // (`grid` workgroups: the host sums `grid` partial slabs per output, groups without a tile write zeros)
      if (a.lw) return h2 ? launch(nm, k_block_bwd_g2<true, false, 1, 2, true>, dim3(grid), dim3(512), lds_g2, st, a)
                          : launch(nm, k_block_bwd_g2<true, false, 1>, dim3(grid), dim3(512), lds_g2, st, a);
      return h2 ? launch(nm, k_block_bwd_g2<false, false, 1, 2, true>, dim3(grid), dim3(512), lds_g2, st, a)
                : launch(nm, k_block_bwd_g2<false, false, 1>, dim3(grid), dim3(512), lds_g2, st, a);
    }
  }
  if (a.lw && !t_ok)
    return fail(FNO_EUNSUPPORTED, "block 0 cannot recompute the lifting in this GEMM mode (the forward pass skipped u_0)");
  if (t_ok) {
    published = a.gmax_out != nullptr;
    if constexpr (C == 32) if (h2) {      // (64 channels: k_block_bwd_g2 above carries the two-term variants)
      GT(2);
      if (a.lw) return launch(nm, k_block_bwd_t<C, 128, false, true, false, 2>, dim3(grid), blk, lds_t, st, a);
      return launch(nm, k_block_bwd_t<C, 128, false, false, false, 2>, dim3(grid), blk, lds_t, st, a);
    }
    GT(3);
    if (a.lw) return launch(nm, k_block_bwd_t<C, 128, false, true>, dim3(grid), blk, lds_t, st, a);
    return launch(nm, k_block_bwd_t<C, 128>, dim3(grid), blk, lds_t, st, a);
  }
  // no fallback behind the exact-fp32 kernel: launch() refuses what exceeds LDS
  const size_t lds = blk_bwd_lds_bytes(C, p->NPX, a);
  GT(1);
  if (p->NPX == 128) return launch(nm, k_block_bwd<C, 128>, dim3(grid), blk, lds, st, a);
  return launch(nm, k_block_bwd<C, 256>, dim3(grid), dim3(BlkBwdCfg<C, 256>::NW * 64), lds, st, a);
}
static int launch_bbwd(const FnoModelPlan* p, hipStream_t st, int grid, const BlkBwdArgs& a, bool* published = nullptr) {
  return p->d.C == 32 ? launch_bbwd_c<32>(p, st, grid, a, published) : launch_bbwd_c<64>(p, st, grid, a, published);
}
static int bbwd_ksplit(const FnoModelPlan* p) {
  const int ntn = p->NPX / 32, mt = p->d.C / 32;
  return ntn / mt;
}
// The projection's forward (no row structure: always 128-pixel tiles).  In this order:
//   k_proj_fwd_w    two fp16 terms     split mode, the bound of |u_L| came (a.xmax), one output channel, whole 32-pixel columns
//   k_proj_fwd_x3   three bf16 terms   split mode otherwise
//   k_proj_fwd      exact fp32
template <int C, int NCO>
static int launch_pfwd_cn(const FnoModelPlan* p, hipStream_t st, int grid, const ProjFwdArgs& a) {
  const size_t lds_w = proj_fwd_w_lds(C, kHID);      // (a constant, 67 KB at 64 channels: its test below is for uniformity only)
  if (g_gemm_x3 && a.xmax && NCO == 1 && a.PW % 32 == 0 && lds_w <= FNO_LDS_MAX) {
    // independent waves, four per SIMD (k_projection_h2.h): two workgroups per CU
    constexpr int NWV = 12;
    const int ncols = a.ntiles * 4;
    constexpr int share_pf = 18;      // of 32; 16 = even (pair_share)
    const int g = std::min((ncols + NWV - 1) / NWV, 2 * p->ncu);
    ProjFwdArgs aw = a;
    aw.share32 = g == 2 * p->ncu ? share_pf : 0;
    return GT(2), launch("k_proj_fwd", k_proj_fwd_w<C, kHID, NWV>, dim3(g), dim3(NWV * 64), lds_w, st, aw);
  }
  if (g_gemm_x3)
    return GT(3), launch("k_proj_fwd", k_proj_fwd_x3<C, kHID, 128, NCO>, dim3(grid), dim3(512), proj_fwd_x3_lds_bytes(C, kHID, NCO), st, a);
  return GT(1), launch("k_proj_fwd", k_proj_fwd<C, kHID, 128, NCO>, dim3(grid), dim3(512), proj_fwd_lds_bytes(C, kHID, NCO), st, a);
}
template <int C>
static int launch_pfwd_c(const FnoModelPlan* p, hipStream_t st, int grid, const ProjFwdArgs& a) {
  return a.CO == 1 ? launch_pfwd_cn<C, 1>(p, st, grid, a) : launch_pfwd_cn<C, PROJ_MAXCO>(p, st, grid, a);
}
template <int C, int NCO>
static int launch_pbwd_cn(const FnoModelPlan* p, hipStream_t st, int grid, const ProjBwdArgs& a) {
  const size_t lds = proj_bwd_lds_bytes(C, kHID, p->NPX, NCO);
  GT(1);
  if (p->NPX == 128) return launch("k_proj_bwd", k_proj_bwd<C, kHID, 128, NCO>, dim3(grid), dim3(512), lds, st, a);
  return launch("k_proj_bwd", k_proj_bwd<C, kHID, 256, NCO>, dim3(grid), dim3(1024), lds, st, a);
}
// second-generation projection backward (k_projection2.h): one output channel, 128-pixel tiles, split-precision mode
static bool use_pbwd_t(int C, int CO, int npx) {
  return g_gemm_x3 && (C == 64 || C == 32) && CO == 1 && npx == 128;
}
// W1 -> bf16x3 fragments in the order k_proj_bwd_t reads them (its two-term fp16 fragments are made by k_absmax3_pack_w1, in the
// launch that scans the bounds)
static int w1_frag_items(int HID, int C) { return (HID / 32) * (C / 16) * 64 + (HID / 32) * 2 * (C / 32) * 64; }
static int pack_w1_x3(hipStream_t st, const float* w1, unsigned short* wa1, unsigned short* wa3, int HID, int C) {
  return launch("k_pack_w1_x3", k_pack_w1_t<3>, dim3((w1_frag_items(HID, C) + 255) / 256), dim3(256), 0, st, w1, wa1, wa3, HID, C,
                (const float*)nullptr);
}
// The projection's backward.  In this order:
//   k_proj_bwd_t   the host packed W1's fragments (a.wa1; use_pbwd_t).  Two fp16 terms when the bounds came (a.amax): NO fallback,
//                  the host has started the gradient-bound chain on it (its carve is at most 132608 bytes: NJ <= 4, W <= 128).
//                  Else three bf16 terms, a third plane per image: with the gradient's row DFT fused (x1g, more than 16 kept
//                  last-dim bins at 64 channels) that carve outgrows LDS, and the next kernel serves
//   k_proj_bwd     exact fp32, first generation (same x1g epilogue, same partial slabs; publishes no bound)
template <int C>
static int launch_pbwd_c(const FnoModelPlan* p, hipStream_t st, int grid, const ProjBwdArgs& a) {
  const size_t lds_t = proj_bwd_t_lds_bytes(C, a);
  if (a.wa1 && use_pbwd_t(C, a.CO, p->NPX)) {
    if (a.amax) return GT(2), launch("k_proj_bwd", k_proj_bwd_t<C, kHID, false, 2>, dim3(grid), dim3(512), lds_t, st, a);
    if (lds_t <= FNO_LDS_MAX) return GT(3), launch("k_proj_bwd", k_proj_bwd_t<C, kHID, false>, dim3(grid), dim3(512), lds_t, st, a);
  }
  return a.CO == 1 ? launch_pbwd_cn<C, 1>(p, st, grid, a) : launch_pbwd_cn<C, PROJ_MAXCO>(p, st, grid, a);
}
static int blk_fwd_grid(const FnoModelPlan* p, int ntiles) {      // persistent grid of the block forwards
  return std::min(ntiles, (g_gemm_x3 ? FNO_GRID_PWX : FNO_GRID_PW) * p->ncu);
}

// spectral middle of one block: x1 -> (hat) -> ohat -> z
static int spectral_mid_fwd(const FnoModelPlan* p, hipStream_t st, int B, const ModelWs& w, const float* wp,
                            float* hat) {
  const Geom& g = p->g;
  const int C = p->d.C;
  if (fused_mid_ok(g, C)) return spectral_mid_fused(st, g, p->t, false, B, C, w.x1, hat, wp, w.z, 0);
  LAUNCHCHK(lead_forward(st, g, p->t, false, B, C, w.x1, w.tmp, hat));
  LAUNCHCHK(mode_gemm(st, hat, wp, w.ohat, B, g.Ktot, C, C, 0));
  return lead_inverse(st, g, p->t, B, C, w.ohat, w.tmp, w.z);
}
// the unfused adjoint middle of nm members (member-major buffers; nm = 1: the model's layer):
//   G = lead_forward(x1) -> ohat ; dW = conj(Xhat) G -> dwp (skipped if null) ; GX = G conj(W) -> hat ; lead_inverse(GX) -> z
// Xhat is shared by the members.  The matrix-core adjoint reads the packed weights wps, the VALU one their transposed copy.
static int spectral_mid_adj(const FnoModelPlan* p, hipStream_t st, const ModelSizes& s, int B, int nm, const float* x1, float* tmp,
                            float* ohat, const float* xhat, float* dwp, const float* wps, const float* wpts, float* hat, float* z) {
  const Geom& g = p->g;
  const int C = p->d.C;
  const bool adj_mfma = mode_gemm_members_ok(C, C);
  const size_t hs = nm > 1 ? s.n_hat : 0, ws = nm > 1 ? s.n_wp : 0;      // member strides
  LAUNCHCHK(lead_forward(st, g, p->t, true, nm * B, C, x1, tmp, ohat));
  if (dwp) LAUNCHCHK(mode_gemm_dw(st, xhat, ohat, dwp, B, g.Ktot, C, C, nm, 0, hs, ws));
  LAUNCHCHK(mode_gemm(st, ohat, adj_mfma ? wps : wpts, hat, B, g.Ktot, C, C, 1, nm, hs, ws, hs, adj_mfma ? 1 : 0));
  return lead_inverse(st, g, p->t, nm * B, C, hat, tmp, z);
}

// one-layer block stacks with a tail (FnoBlockTail, include/fnoengine.h): what the plan must look like
static int tail_check(const FnoModelPlan* p, const FnoBlockTail* t, bool backward) {
  if (!t) return FNO_OK;
  const FnoModelDesc& d = p->d;
  if (d.Cin != 0 || d.Cout != 0 || d.n_layers != 1) return fail(FNO_EUNSUPPORTED, "block tail: one-layer block stacks only");
  if (p->NPX != 128 || p->loose || !row_fast_ok(p->g, d.C))
    return fail(FNO_EUNSUPPORTED, "block tail: 32 / 64 channels, rows of 32 / 64 / 128 floats");
  if (t->drop_p < 0.f || t->drop_p >= 1.f) return fail(FNO_EINVAL, "block tail: dropout rate %g outside [0, 1)", (double)t->drop_p);
  if (t->drop_p > 0.f && !t->drop_seed) return fail(FNO_EINVAL, "block tail: dropout needs the two seed words (device pointer)");
  if (backward && t->relu_out && !t->y) return fail(FNO_EINVAL, "block tail: the backward of a ReLU tail needs the forward's output");
  return FNO_OK;
}
static int model_forward_impl(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x, float* y,
                              void* saved, void* ws, size_t ws_bytes, void* stream, const FnoBlockTail* tail);
extern "C" int fno_model_forward(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x, float* y,
                                 void* saved, void* ws, size_t ws_bytes, void* stream) {
  return model_forward_impl(p, B, prm, x, y, saved, ws, ws_bytes, stream, nullptr);
}
extern "C" int fno_model_forward_tail(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x, float* y,
                                      void* saved, void* ws, size_t ws_bytes, void* stream, const FnoBlockTail* tail) {
  if (!tail) return fail(FNO_EINVAL, "fno_model_forward_tail: null tail");
  return model_forward_impl(p, B, prm, x, y, saved, ws, ws_bytes, stream, tail);
}
static int model_forward_impl(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x, float* y,
                              void* saved, void* ws, size_t ws_bytes, void* stream, const FnoBlockTail* tail) {
  if (!p || !prm || !x || !y || B < 1) return fail(FNO_EINVAL, "fno_model_forward: bad argument");
  if (!saved) return fail(FNO_EINVAL, "fno_model_forward: `saved` buffer required (fno_model_saved_bytes)");
  LAUNCHCHK(tail_check(p, tail, false));
  hipStream_t st = (hipStream_t)stream;
  const Geom& g = p->g;
  const FnoModelDesc& d = p->d;
  const int C = d.C, L = d.n_layers;
  const ModelSizes s = model_sizes(p, B);
  bool ok;
  ModelWs w = carve_model(p, B, ws, ws_bytes, false, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  const ModelSaved sv = carve_saved(p, B, saved);
  float* const u = sv.u;
  float* const amax = sv.bounds;
  // The ONE two-term decision of the forward: two-term fp16 GEMMs with published magnitude bounds from 1024 tiles up - below
  // that the kernels are latency-bound and the bound bookkeeping (one more launch, the weight scans in the prologues) costs
  // more than three matrix products save (BASELINE config 1, 128 tiles: 0.27 -> 0.22 ms per step without it)
  const bool h2 = g_gemm_x3 && d.Cout > 0 && (size_t)B * g.PW >= ((size_t)1 << 17);
  static_assert(kNAmax == 64, "k_pack_w_tiled clears 64 slots");
  // (the bound slots are cleared by the weight pack's first workgroup - the first launch of the pass - or, plane-major weights, by a fill)
  // the matrix-core adjoint reads wps; the fused middle's adjoint streams the transposed copy
  LAUNCHCHK(pack_w_layers(st, g, C, C, corner_ptrs<CornerPtrsL>(g, prm->spec_w, 0, L - 1), L, sv.wps,
                          mode_gemm_members_ok(C, C) && !fused_mid_shape_ok(g, C) ? nullptr : sv.wpts, s.n_wp, h2 ? amax : nullptr));

  const bool has_lift = d.Cin > 0, has_proj = d.Cout > 0;
  bool lift_xmax = false;      // max |x| of the model input was published (k_lift_rowdft)
  bool u0_bound = false;       // block 0's forward published the bound of |u_0| (bnd_u(0))
  FnoModelPlan::CallState cs;
  cs.B = B;
  PwFwdArgs a;
  if (has_lift) {
    // lifting (tfno.py:19-20) + row DFT of its output
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = prm->lift_w; a.bias = prm->lift_b;
    cs.u0_skipped = lift_fused(p);
    a.u = cs.u0_skipped ? nullptr : u; a.x1 = p->loose ? nullptr : w.x1; a.tfwd = p->t.tfwd_f;
    set_tile_geom(a, g, s, 0);
    const size_t lds_lr = ((size_t)2 * g.Klast * (g.W + 4) + (size_t)LR_ROWS * d.Cin * (g.W + 4) + 2) * 4 + (size_t)LR_ROWS * g.Klast * (d.Cin + 1) * 8;
    if (cs.u0_skipped && !p->loose && lds_lr <= 48 * 1024) {
      // u_0 is never stored: only its row spectra are needed, and those are linear in the <= 4 input channels
      const int nrows = B * g.P;
      LAUNCHCHK(launch("k_lift_rowdft", k_lift_rowdft, dim3((nrows + LR_ROWS - 1) / LR_ROWS), dim3(256), lds_lr, st, x,
                       prm->lift_w, prm->lift_b, p->t.tfwd_f, (float2*)w.x1, d.Cin, C, g.PW, g.W, g.P, g.Klast, nrows,
                       h2 ? amax + kBndX : nullptr));
      lift_xmax = h2;
    } else
    LAUNCHCHK(launch_lift(p, st, std::min(s.ntiles, FNO_GRID_LIFT * p->ncu), a));
    if (p->loose) LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, C, u, w.x1));   // no epilogue on loose rows
  } else if (tail && tail->drop_p > 0.f) {
    RowMod mod;                          // the spectral branch sees drop(x) (rno.py:98); the skip branch below reads x itself
    mod.drop_seed = tail->drop_seed; mod.drop_p = tail->drop_p;
    LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, C, x, w.x1, 0, &mod));
  } else {
    LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, C, x, w.x1));     // block stack: x is u_0
  }

  for (int l = 0; l < L; ++l) {
    if (p->loose && l > 0)     // no row-DFT epilogue on loose rows: transform act(u_l) in its own pass
      LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, C, u + (size_t)l * s.n_act, w.x1,
                            (int)((d.gelu_mask >> (l - 1)) & 1u)));
    LAUNCHCHK(spectral_mid_fwd(p, st, B, w, sv.wps + (size_t)l * s.n_wp, sv.hats + (size_t)l * s.n_hat));
    memset(&a, 0, sizeof(a));
    a.x = (l == 0 && !has_lift) ? x : u + (size_t)l * s.n_act;
    if (l == 0 && has_lift && cs.u0_skipped) { a.x = x; a.lw = prm->lift_w; a.lb = prm->lift_b; a.CL = d.Cin; }
    a.w = prm->skip_w[l];
    a.bias = prm->spec_bias ? prm->spec_bias + (size_t)l * C : nullptr;
    a.z = w.z; a.tinv = p->t.tinv_f;
    a.u = (l == L - 1 && !has_proj) ? y : u + (size_t)(l + 1) * s.n_act;
    a.x1 = (l + 1 < L && !p->loose) ? w.x1 : nullptr;
    a.tfwd = p->t.tfwd_f;
    set_tile_geom(a, g, s, g.Klast);
    a.act_in = (l > 0) && ((d.gelu_mask >> (l - 1)) & 1u);
    a.act_out = (d.gelu_mask >> l) & 1u;
    a.relu_out = tail && tail->relu_out;
    if (h2) {      // magnitude bounds for the two-term fp16 GEMMs: every block publishes max |u_{l+1}| for its consumer
      // (measured at 32 channels, FNO3d 64^3: tracking the maximum costs k_pw_fwd_x3 0.012 ms per launch, the fp16 products
      // it enables save the block backward 0.017 ms per launch)
      a.umax = amax + bnd_u(l + 1);
      if (l == 0) { a.xmax = (a.lw && lift_xmax) ? amax + kBndX : nullptr; a.ubound = amax + bnd_u(0); }   // (an unfused u_0 has no published bound)
      else a.xmax = amax + bnd_u(l);
    }
    // zigzag: every block walks its tiles in the opposite direction of its producer, so that it starts on the part of its
    // input the producer wrote last - what the 256 MB Infinity Cache still holds of it (kernels without the option walk forward)
    a.rev = g_zigzag ? (l & 1) : 0;
    bool ub = false;
    LAUNCHCHK(launch_block(p, st, blk_fwd_grid(p, s.ntiles), a, &ub));
    if (l == 0) u0_bound = ub;
  }

  if (!has_proj) { p->put_call(saved, cs); return FNO_OK; }
  // projection (tfno.py:34-38)
  ProjFwdArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.x = u + (size_t)L * s.n_act; pa.w1 = prm->proj_w1; pa.b1 = prm->proj_b1; pa.w2 = prm->proj_w2; pa.b2 = prm->proj_b2;
  pa.y = y; pa.PW = g.PW; pa.CO = d.Cout; pa.act_in = (d.gelu_mask >> (L - 1)) & 1u;
  pa.tiles_per_plane = g.PW / 128; pa.ntiles = B * pa.tiles_per_plane;
  pa.xmax = h2 ? amax + bnd_u(L) : nullptr;
  cs.h2_fwd = h2;
  cs.bwd_clean = h2;
  cs.h2_u0 = lift_xmax && u0_bound;      // (both need h2; else the three-term block-0 backward, which needs no bound)
  p->put_call(saved, cs);
  const int pgrid = std::min(pa.ntiles, FNO_GRID_PF * p->ncu);
  if (C == 32) LAUNCHCHK(launch_pfwd_c<32>(p, st, pgrid, pa));
  else LAUNCHCHK(launch_pfwd_c<64>(p, st, pgrid, pa));
  return FNO_OK;
}

extern "C" int fno_model_backward(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                                  const float* dy, const void* saved, const FnoModelGrads* gr, void* ws,
                                  size_t ws_bytes, void* stream) {
  return fno_model_backward_dx(p, B, prm, x, dy, saved, gr, nullptr, ws, ws_bytes, stream);
}
extern "C" int fno_model_backward_dx(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                                     const float* dy, const void* saved, const FnoModelGrads* gr, float* dx, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (!p) return fail(FNO_EINVAL, "fno_model_backward: bad argument");
  return fno_model_backward_part(p, B, prm, x, dy, saved, gr, dx, ws, ws_bytes, stream, p->d.n_layers - 1, 0);
}
// Layers l_hi .. l_lo (descending) of the backward pass; l_hi == n_layers-1 includes the projection, l_lo == 0 the
// lifting.  Consecutive calls over a partition of the layers with the SAME workspace reproduce the full pass bit for
// bit (the running gradient and its row spectrum live in the workspace); every call finishes the gradients of its own
// layers (slab reduction + weight unpack), so a data-parallel caller can start exchanging them while the rest runs.
static int model_backward_impl(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                               const float* dy, const void* saved, const FnoModelGrads* gr, float* dx, void* ws,
                               size_t ws_bytes, void* stream, int l_hi, int l_lo, const FnoBlockTail* tail);
extern "C" int fno_model_backward_part(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                                       const float* dy, const void* saved, const FnoModelGrads* gr, float* dx, void* ws,
                                       size_t ws_bytes, void* stream, int l_hi, int l_lo) {
  return model_backward_impl(p, B, prm, x, dy, saved, gr, dx, ws, ws_bytes, stream, l_hi, l_lo, nullptr);
}
extern "C" int fno_model_backward_tail(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                                       const float* dy, const void* saved, const FnoModelGrads* gr, float* dx, void* ws,
                                       size_t ws_bytes, void* stream, const FnoBlockTail* tail) {
  if (!p || !tail) return fail(FNO_EINVAL, "fno_model_backward_tail: null argument");
  return model_backward_impl(p, B, prm, x, dy, saved, gr, dx, ws, ws_bytes, stream, p->d.n_layers - 1, 0, tail);
}
static int model_backward_impl(const FnoModelPlan* p, int B, const FnoModelParams* prm, const float* x,
                               const float* dy, const void* saved, const FnoModelGrads* gr, float* dx, void* ws,
                               size_t ws_bytes, void* stream, int l_hi, int l_lo, const FnoBlockTail* tail) {
  if (!p || !prm || !x || !dy || !saved || !gr || B < 1) return fail(FNO_EINVAL, "fno_model_backward: bad argument");
  LAUNCHCHK(tail_check(p, tail, true));
  if (dx && p->d.Cin > 4) return fail(FNO_EUNSUPPORTED, "input gradient through the lifting layer: at most 4 input channels");
  if (l_lo < 0 || l_hi >= p->d.n_layers || l_lo > l_hi) return fail(FNO_EINVAL, "fno_model_backward_part: layers %d..%d", l_hi, l_lo);
  hipStream_t st = (hipStream_t)stream;
  const Geom& g = p->g;
  const FnoModelDesc& d = p->d;
  const int C = d.C, L = d.n_layers;
  const ModelSizes s = model_sizes(p, B);
  bool ok;
  ModelWs w = carve_model(p, B, ws, ws_bytes, true, &ok);
  if (!ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  const ModelSaved sv = carve_saved(p, B, saved);
  const float *u = sv.u, *hats = sv.hats;
  float* const amax = sv.bounds;
  const bool fused_mid = fused_mid_ok(g, C);           // the forward packed the transposed copy as well
  if (!mode_gemm_members_ok(C, C) && !fused_mid_shape_ok(g, C))       // VALU contraction (A/B switch): the forward may have skipped the transposed copy
    LAUNCHCHK(pack_w_layers(st, g, C, C, corner_ptrs<CornerPtrsL>(g, prm->spec_w, l_lo, l_hi), l_hi - l_lo + 1, nullptr,
                            sv.wpts + (size_t)l_lo * s.n_wp, s.n_wp));
  JobList jobs;

  const bool has_lift = d.Cin > 0, has_proj = d.Cout > 0;
  bool cs_found = false;
  FnoModelPlan::CallState cs = p->get_call(saved, B, &cs_found);      // what the forward pass that filled `saved` published
  if (!cs_found) {
    // an unknown buffer: u_0 was written or not exactly as a forward of this plan decides it (a default of "written" would let
    // block 0 read memory the forward never filled); no bounds are assumed published
    static const int strict = getenv("FNO_STRICT_SAVED") ? 1 : 0;
    if (strict) return fail(FNO_EINVAL, "fno_model_backward: `saved` buffer %p was not filled by a forward pass of this plan", saved);
    cs.u0_skipped = has_lift && lift_fused(p);
  }
  cs.B = B;
  // The two-term decisions of this pass (fno_dev.h "h2"), made here once.  The forward pass of THIS buffer published max |u_l| and
  // the mode allows two-term: the block kernels may take their fp16 variants (each needs its input gradient's bound too: gvalid)
  const bool h2_chain = g_gemm_x3 && cs.h2_fwd;
  // ... and the projection backward has a two-term kernel for this plan: it scans its scalars' bounds and starts the chain
  const bool h2_proj = h2_chain && use_pbwd_t(C, d.Cout, p->NPX);
  bool gvalid = false;      // amax[bnd_g(l + 1)] bounds the gradient the next block kernel reads
  if (l_hi < L - 1 && h2_chain) gvalid = cs.gchain_valid;      // a later part: left by the previous part's last kernel
  // ---- projection backward -> gA = dL/du_L, row DFT (gradient tables) -> x1 ----
  ProjBwdArgs pb;
  memset(&pb, 0, sizeof(pb));
  if (l_hi < L - 1) {
    // a later part: the running gradient and its row spectrum were left in the workspace by the previous call
  } else if (!has_proj && tail && tail->relu_out) {
    // dy is dL/d relu(u_L): the row pass applies the derivative (mask read off the forward's output) and leaves
    // g = dL/du_L in the workspace for the block kernel
    RowMod mod;
    mod.ymask = tail->y; mod.gmasked = w.ga;
    LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, dy, w.x1, 0, &mod));
  } else if (!has_proj) {
    LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, dy, w.x1));     // dy is dL/du_L
  } else {
  // Bound slots written by the backward pass: bnd_g(l) (the chain) and the projection's scalars behind kBndProj - ONE contiguous
  // range, [bnd_g(0), kNAmax), cleared by ONE memset at the start of the pass (round 3 issued five small ones per step; the
  // forward's clearing of all slots is the other one) whenever any of its slots is written in this pass: a second backward on
  // the same `saved` must not keep the first one's.  (Not after a forward that has just cleared all slots: one 4.5 us fill
  // less per step; a second backward on the same `saved`, or an unknown buffer, clears.)
  bool db2_done = false;
  if (h2_chain && !(cs_found && cs.bwd_clean) &&
      hipMemsetAsync(amax + bnd_g(0), 0, (kNAmax - bnd_g(0)) * sizeof(float), st) != hipSuccess)
    return fail(FNO_EHIP, "memset of the magnitude bounds");
  if (use_pbwd_t(C, d.Cout, p->NPX)) {      // (split mode, one output channel: k_proj_bwd_t reads W1 as packed fragments)
    if (h2_proj) {
      // the scan of max |dy|, max |W1|, max |w2| and the split of W1 into its two fp16 terms share a launch, which also leaves
      // 256 partial sums of dy = the bias gradient's partial slabs (one output channel; k_channel_sums below is then not launched)
      static_assert(kBndW1 == kBndDy + 1 && kBndW2 == kBndDy + 2, "k_absmax3_pack_w1 writes three consecutive slots");
      db2_done = true;
      LAUNCHCHK(launch("k_absmax", k_absmax3_pack_w1, dim3(256 + 8 + 1 + (w1_frag_items(kHID, C) + 255) / 256), dim3(256), 0, st, dy,
                       (size_t)B * d.Cout * g.PW, 256, prm->proj_w1, 8, prm->proj_w2, (size_t)d.Cout * kHID, 1, amax + kBndDy,
                       w.db2_part, w.wa1, w.wa3, kHID, C));
      pb.amax = amax + kBndProj; pb.xmax = amax + bnd_u(L);
      pb.gmax_out = amax + bnd_g(L);      // the chain of gradient bounds starts here
      gvalid = true;
    } else LAUNCHCHK(pack_w1_x3(st, prm->proj_w1, w.wa1, w.wa3, kHID, C));
    pb.wa1 = w.wa1; pb.wa3 = w.wa3;
  }
  pb.x = u + (size_t)L * s.n_act; pb.dy = dy; pb.w1 = prm->proj_w1; pb.b1 = prm->proj_b1;
  pb.w2 = prm->proj_w2; pb.gout = w.ga; pb.x1g = p->loose ? nullptr : w.x1; pb.tfwd = p->t.tfwd_b;
  pb.dw1_part = w.dw1_part; pb.db1_part = w.db1_part; pb.dw2_part = w.dw2_part;
  pb.PW = g.PW; pb.W = g.W; pb.P = g.P; pb.K2out = g.Klast; pb.NJ = g.NJ; pb.CO = d.Cout;
  pb.act_in = (d.gelu_mask >> (L - 1)) & 1u;
  pb.tiles_per_plane = s.tiles_per_plane; pb.ntiles = s.ntiles;
  pb.rev = g_zigzag;      // the forward pass's projection read u_L front to back: start at the back (k_proj_bwd_t; the others ignore it)
  if (C == 32) LAUNCHCHK(launch_pbwd_c<32>(p, st, s.grid, pb));
  else LAUNCHCHK(launch_pbwd_c<64>(p, st, s.grid, pb));
  jobs.add(w.dw1_part, gr->proj_w1, s.grid, kHID, C, C, C);
  const int pslabs = p->NPX / 32;      // db1 / dW2 partial slabs per workgroup
  jobs.add(w.db1_part, gr->proj_b1, s.grid * pslabs, 1, kHID, kHID, kHID);
  jobs.add(w.dw2_part, gr->proj_w2, s.grid * pslabs, d.Cout, kHID, kHID, kHID);
  if (!db2_done) LAUNCHCHK(launch("k_channel_sums", k_channel_sums, dim3(64, d.Cout), dim3(256), 0, st, dy, w.db2_part, B, d.Cout, g.PW));
  jobs.add(w.db2_part, gr->proj_b2, db2_done ? 256 : 64, 1, d.Cout, d.Cout, d.Cout);
  if (p->loose) LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, w.ga, w.x1));   // dL/du_L's row spectrum
  }

  const float* gcur = (has_proj || (tail && tail->relu_out)) ? w.ga : dy;   // dL/du_{l+1}
  float* gnext = has_proj ? w.gb : w.ga;
  float* gspare = has_proj ? w.ga : w.gb;
  for (int l = L - 1; l > l_hi; --l) {        // replay the buffer rotation of the layers done by earlier parts
    gcur = gnext;
    float* t = gnext; gnext = gspare; gspare = t;
  }
  const int ks = bbwd_ksplit(p);
  const bool batch_dw = l_hi > l_lo && mode_gemm_members_ok(C, C) && !(B <= 4 && (long)g.Ktot * C * C >= (1L << 21));
  for (int l = l_hi; l >= l_lo; --l) {
    // spectral backward middle: G = lead_forward(x1) ; dW = conj(Xhat) G ; GX = G conj(W) ; zg = lead_inverse(GX)
    float* dwp_l = w.dwp + (size_t)l * s.n_wp;
    float* dw_part_l = w.dw_part + (size_t)l * s.grid_bb * ks * C * C;
    float* db_part_l = w.db_part + (size_t)l * s.grid_bb * C;
    // G_l is kept per layer: dW_l = conj(Xhat_l) G_l does not feed the dx chain, so all layers of this part share ONE
    // contraction launch behind the loop (layer index on the grid) instead of one 72-workgroup launch each
    float* ohat_l = w.ohat + (size_t)(batch_dw ? l : 0) * s.n_hat;
    if (fused_mid) {
      LAUNCHCHK(spectral_mid_fused(st, g, p->t, true, B, C, w.x1, ohat_l, sv.wpts + (size_t)l * s.n_wp, w.z, 1));
      if (!batch_dw) LAUNCHCHK(mode_gemm_dw(st, hats + (size_t)l * s.n_hat, ohat_l, dwp_l, B, g.Ktot, C, C));
    } else
      LAUNCHCHK(spectral_mid_adj(p, st, s, B, 1, w.x1, w.tmp, ohat_l, hats + (size_t)l * s.n_hat, batch_dw ? nullptr : dwp_l,
                                 sv.wps + (size_t)l * s.n_wp, sv.wpts + (size_t)l * s.n_wp, w.hat, w.z));

    BlkBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.g = gcur; a.uin = (l == 0 && !has_lift) ? x : u + (size_t)l * s.n_act; a.w = prm->skip_w[l];
    a.zg = w.z; a.tinv = p->t.tinv_b;
    a.gout = (l > 0) ? gnext : (has_lift ? (dx ? gnext : nullptr) : dx);     // dx through a lifting layer: dL/du_0 is needed
    a.x1g = (l > 0 && !p->loose) ? w.x1 : nullptr;
    a.tfwd = p->t.tfwd_b;
    a.dw_part = dw_part_l; a.db_part = db_part_l;
    a.xin = (l == 0 && has_lift) ? x : nullptr; a.dwl_part = w.dwl_part; a.CL = d.Cin;
    if (l == 0 && has_lift && cs.u0_skipped) { a.lw = prm->lift_w; a.lb = prm->lift_b; }
    set_tile_geom(a, g, s, g.Klast);
    a.act_in = (l > 0) && ((d.gelu_mask >> (l - 1)) & 1u);
    if (tail && tail->drop_p > 0.f) { a.drop_seed = tail->drop_seed; a.drop_p = tail->drop_p; }
    if (h2_chain) {
      // bounds for the two-term fp16 GEMMs: |g| from the previous kernel of the chain, |u_l| from the forward pass
      if (gvalid && (l > 0 || (a.lw && cs.h2_u0))) { a.gmax_in = amax + bnd_g(l + 1); a.umax = amax + bnd_u(l); }
      if (l > 0) a.gmax_out = amax + bnd_g(l);      // (cleared with the whole range at the start of the pass)
    }
    a.rev = g_zigzag ? ((L - 1 - l) & 1) : 0;      // zigzag along the chain: the projection backward ended at the front
    bool published = false;
    LAUNCHCHK(launch_bbwd(p, st, s.grid_bb, a, &published));
    gvalid = published;
    if (p->loose && l > 0)     // the running gradient's row spectrum for the next (lower) block, in its own pass
      LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, gnext, w.x1));
    jobs.add(dw_part_l, gr->skip_w[l], s.grid_bb * ks, C, C, C, C);
    if (gr->spec_bias) jobs.add(db_part_l, gr->spec_bias + (size_t)l * C, s.grid_bb, 1, C, C, C);
    if (l == 0 && has_lift) {
      jobs.add(w.dwl_part, gr->lift_w, s.grid_bb, C, d.Cin, 16, d.Cin);
      jobs.add(w.dwl_part + d.Cin, gr->lift_b, s.grid_bb, C, 1, 16, 1);
    }
    gcur = gnext;
    { float* t = gnext; gnext = gspare; gspare = t; }
  }
  cs.gchain_valid = gvalid;
  cs.bwd_clean = false;
  p->put_call(saved, cs);
  if (dx && has_lift && l_lo == 0) {      // dL/dx = W_l^T dL/du_0 (gcur is block 0's output gradient after the rotation)
    const size_t n4 = (size_t)B * g.PW / 4;
    LAUNCHCHK(launch("k_lift_dx", k_lift_dx, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 8192)), dim3(256), 0, st, gcur,
                     prm->lift_w, dx, C, d.Cin, (size_t)g.PW, n4));
  }
  if (batch_dw)
    LAUNCHCHK(mode_gemm_dw(st, hats + (size_t)l_lo * s.n_hat, w.ohat + (size_t)l_lo * s.n_hat, w.dwp + (size_t)l_lo * s.n_wp, B,
                           g.Ktot, C, C, l_hi - l_lo + 1, s.n_hat, s.n_hat, s.n_wp));
  LAUNCHCHK(jobs.run(st));
  // packed dW of this part's layers -> the corner gradients
  return unpack_dw_layers(st, g, C, C, w.dwp + (size_t)l_lo * s.n_wp, corner_ptrs<CornerPtrsMutL>(g, gr->spec_w, l_lo, l_hi),
                          l_hi - l_lo + 1, s.n_wp);
}

// ===========================================================================
// Fan-out of Fourier layers over ONE input (neuralop/models/rno.py:254-260: f1, f3, f5, f7 act on x, f2, f4, f8 on h):
//   y_j = SpecConv_j(x) + W_j x + b_j,  j < n_out,
// on a block-stack plan (Cin = Cout = 0, no GELU) created with n_layers >= n_out (sizes the workspace).  The forward row
// transform and leading-axis passes of x run once for all members; backward chains the members' input gradients through
// the block kernel's gradient-addend input (dx is read and rewritten in place), so no accumulation pass exists.
// Members use layer slots 0..n_out-1 of FnoModelParams / FnoModelGrads (skip_w, spec_w); biases come as separate (C) arrays.
// ===========================================================================
static int fanout_check(const FnoModelPlan* p, int B, int n_out) {
  if (!p || B < 1) return fail(FNO_EINVAL, "fno_fanout: bad argument");
  if (p->d.Cin != 0 || p->d.Cout != 0 || p->d.gelu_mask != 0)
    return fail(FNO_EINVAL, "fno_fanout: needs a block-stack plan (Cin = Cout = 0) without activations");
  if (n_out < 1 || n_out > p->d.n_layers) return fail(FNO_EINVAL, "fno_fanout: %d members on a plan sized for %d", n_out, p->d.n_layers);
  return FNO_OK;
}
// every member's contraction and leading-axis passes in one launch each
static bool fanout_batched(const FnoModelPlan* p, int B, int n_out) {
  return n_out > 1 && mode_gemm_members_ok(p->d.C, p->d.C) && (long)n_out * B * (p->g.nlead == 2 ? p->g.dims[0] : 1) <= 65535;
}
extern "C" size_t fno_fanout_saved_bytes(const FnoModelPlan* p, int B, int n_out) {
  if (!p || B < 1 || n_out < 1) return 0;
  const ModelSizes s = model_sizes(p, B);
  return (s.n_hat + (size_t)2 * n_out * s.n_wp) * sizeof(float) + 256;
}
// member-major copies of the spectral-middle buffers, so that the leading-axis passes and the mode contractions of all
// members run as ONE launch each (outer dimension n_out * B; member index on the contraction grid)
struct FanWs { float *x1, *z, *ohat, *hat2, *tmp; size_t total; bool ok; };
static FanWs carve_fanout(const FnoModelPlan* p, int B, int n_out, void* ws, size_t cap, size_t base) {
  const ModelSizes s = model_sizes(p, B);
  Carver c(ws ? (char*)ws + base : nullptr, cap > base ? cap - base : 0);
  FanWs f;
  f.x1 = c.take<float>((size_t)n_out * s.n_x1);
  f.z = c.take<float>((size_t)n_out * s.n_x1);
  f.ohat = c.take<float>((size_t)n_out * s.n_hat);
  f.hat2 = c.take<float>((size_t)n_out * s.n_hat);
  f.tmp = c.take<float>((size_t)n_out * s.n_tmp);
  f.total = base + c.off;
  f.ok = c.ok;
  return f;
}
extern "C" size_t fno_fanout_workspace_bytes(const FnoModelPlan* p, int B, int n_out) {
  if (!p || B < 1 || n_out < 1) return 0;
  const size_t base = carve_model(p, B, nullptr, 0, true, nullptr).total;
  return carve_fanout(p, B, n_out, nullptr, 0, base).total;
}
extern "C" int fno_fanout_forward(const FnoModelPlan* p, int B, int n_out, const FnoModelParams* prm,
                                  const float* const* bias, const float* x, float* const* y, void* saved, void* ws,
                                  size_t ws_bytes, void* stream) {
  LAUNCHCHK(fanout_check(p, B, n_out));
  if (!prm || !x || !y || !saved) return fail(FNO_EINVAL, "fno_fanout_forward: null argument");
  hipStream_t st = (hipStream_t)stream;
  const Geom& g = p->g;
  const int C = p->d.C;
  const ModelSizes s = model_sizes(p, B);
  bool ok;
  ModelWs w = carve_model(p, B, ws, ws_bytes, true, &ok);
  FanWs f = carve_fanout(p, B, n_out, ws, ws_bytes, w.total);
  if (!ok || !f.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu (fno_fanout_workspace_bytes)", f.total, ws_bytes);
  float* hat = (float*)saved;
  float* wps = hat + s.n_hat;
  float* wpts = wps + (size_t)n_out * s.n_wp;
  LAUNCHCHK(pack_w_layers(st, g, C, C, corner_ptrs<CornerPtrsL>(g, prm->spec_w, 0, n_out - 1), n_out, wps,
                          mode_gemm_members_ok(C, C) ? nullptr : wpts, s.n_wp));
  LAUNCHCHK(row_forward(st, g, p->t.tfwd_f, p->t.tT[0], p->t.K2P, B, C, x, w.x1));
  LAUNCHCHK(lead_forward(st, g, p->t, false, B, C, w.x1, w.tmp, hat));        // the shared truncated spectrum of x
  const bool batched = fanout_batched(p, B, n_out);
  if (batched) {
    LAUNCHCHK(mode_gemm(st, hat, wps, f.ohat, B, g.Ktot, C, C, 0, n_out, 0, s.n_wp, s.n_hat));
    LAUNCHCHK(lead_inverse(st, g, p->t, n_out * B, C, f.ohat, f.tmp, f.z));
  }
  for (int j = 0; j < n_out; ++j) {
    if (!y[j]) return fail(FNO_EINVAL, "fno_fanout_forward: y[%d] is null", j);
    const float* zj = w.z;
    if (batched) zj = f.z + (size_t)j * s.n_x1;
    else {
      LAUNCHCHK(mode_gemm(st, hat, wps + (size_t)j * s.n_wp, w.ohat, B, g.Ktot, C, C, 0));
      LAUNCHCHK(lead_inverse(st, g, p->t, B, C, w.ohat, w.tmp, w.z));
    }
    PwFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = prm->skip_w[j]; a.bias = bias ? bias[j] : nullptr;
    a.z = zj; a.tinv = p->t.tinv_f; a.u = y[j]; a.tfwd = p->t.tfwd_f;
    set_tile_geom(a, g, s, g.Klast);
    LAUNCHCHK(launch_block(p, st, blk_fwd_grid(p, s.ntiles), a));
  }
  return FNO_OK;
}
extern "C" int fno_fanout_backward(const FnoModelPlan* p, int B, int n_out, const FnoModelParams* prm, const float* x,
                                   const float* const* dy, const void* saved, const FnoModelGrads* gr,
                                   float* const* dbias, float* dx, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(fanout_check(p, B, n_out));
  if (!prm || !x || !dy || !saved || !gr || !dx) return fail(FNO_EINVAL, "fno_fanout_backward: null argument");
  hipStream_t st = (hipStream_t)stream;
  const Geom& g = p->g;
  const int C = p->d.C;
  const ModelSizes s = model_sizes(p, B);
  bool ok;
  ModelWs w = carve_model(p, B, ws, ws_bytes, true, &ok);
  FanWs f = carve_fanout(p, B, n_out, ws, ws_bytes, w.total);
  if (!ok || !f.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu (fno_fanout_workspace_bytes)", f.total, ws_bytes);
  const float* hat = (const float*)saved;
  const float* wps = hat + s.n_hat;
  float* wpts = const_cast<float*>(wps) + (size_t)n_out * s.n_wp;
  if (!mode_gemm_members_ok(C, C))      // VALU contraction: the forward skipped the transposed copy
    LAUNCHCHK(pack_w_layers(st, g, C, C, corner_ptrs<CornerPtrsL>(g, prm->spec_w, 0, n_out - 1), n_out, nullptr, wpts, s.n_wp));
  const int ks = bbwd_ksplit(p);
  for (int j = 0; j < n_out; ++j)
    if (!dy[j]) return fail(FNO_EINVAL, "fno_fanout_backward: dy[%d] is null", j);
  const bool batched = fanout_batched(p, B, n_out);
  if (batched) {
    for (int j = 0; j < n_out; ++j)
      LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, dy[j], f.x1 + (size_t)j * s.n_x1));
    LAUNCHCHK(spectral_mid_adj(p, st, s, B, n_out, f.x1, f.tmp, f.ohat, hat, w.dwp, wps, wpts, f.hat2, f.z));
  }
  JobList jobs;
  for (int j = 0; j < n_out; ++j) {
    float* dwp_j = w.dwp + (size_t)j * s.n_wp;
    float* dw_part_j = w.dw_part + (size_t)j * s.grid_bb * ks * C * C;
    float* db_part_j = w.db_part + (size_t)j * s.grid_bb * C;
    const float* zj = w.z;
    if (batched) zj = f.z + (size_t)j * s.n_x1;
    else {
      LAUNCHCHK(row_forward(st, g, p->t.tfwd_b, p->t.tT[1], p->t.K2P, B, C, dy[j], w.x1));
      LAUNCHCHK(spectral_mid_adj(p, st, s, B, 1, w.x1, w.tmp, w.ohat, hat, dwp_j, wps + (size_t)j * s.n_wp, wpts + (size_t)j * s.n_wp,
                                 w.hat, w.z));
    }
    BlkBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dy[j]; a.uin = x; a.w = prm->skip_w[j];
    a.zg = zj; a.tinv = p->t.tinv_b;
    a.gout = dx; a.gadd = j > 0 ? dx : nullptr;          // every lane re-reads exactly the elements it then rewrites
    a.tfwd = p->t.tfwd_b;
    a.dw_part = dw_part_j; a.db_part = db_part_j;
    set_tile_geom(a, g, s, g.Klast);
    LAUNCHCHK(launch_bbwd(p, st, s.grid_bb, a));
    jobs.add(dw_part_j, gr->skip_w[j], s.grid_bb * ks, C, C, C, C);
    if (dbias && dbias[j]) jobs.add(db_part_j, dbias[j], s.grid_bb, 1, C, C, C);
  }
  LAUNCHCHK(jobs.run(st));
  return unpack_dw_layers(st, g, C, C, w.dwp, corner_ptrs<CornerPtrsMutL>(g, gr->spec_w, 0, n_out - 1), n_out, s.n_wp);
}

// ===========================================================================
// Training-step tail: fused decode + LpLoss.rel (+ gradient) and Adam on a flat bucket
// ===========================================================================
static const int kLossSplit = 16;
extern "C" size_t fno_lploss_workspace_bytes(int batch) {
  return ((size_t)batch * kLossSplit * 2 + (size_t)batch) * sizeof(float);
}
extern "C" int fno_lploss_rel_forward(int batch, size_t n, const float* pred, const float* target, const float* mean,
                                      const float* stdv, int stat_len, float eps, int size_average, float* loss,
                                      void* ws, size_t ws_bytes, void* stream) {
  if (batch < 1 || n < 1 || !pred || !target || !loss || !ws) return fail(FNO_EINVAL, "fno_lploss_rel_forward: bad argument");
  if ((mean || stdv) && stat_len != 1 && (size_t)stat_len != n)
    return fail(FNO_EINVAL, "decode statistics must have 1 or %zu elements, got %d", n, stat_len);
  if (ws_bytes < fno_lploss_workspace_bytes(batch))
    return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", fno_lploss_workspace_bytes(batch), ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
  float* coef = partial + (size_t)batch * kLossSplit * 2;
  LAUNCHCHK(launch("k_lploss_partial", k_lploss_partial, dim3(kLossSplit, batch), dim3(256), 0, st, pred, target, mean, stdv,
                   stat_len, eps, n, partial));
  LAUNCHCHK(launch("k_lploss_finish", k_lploss_finish, dim3(1), dim3(256), 0, st, (const float*)partial, batch, kLossSplit,
                   size_average ? 1.0f / (float)batch : 1.0f, loss, coef));
  return FNO_OK;
}
extern "C" int fno_lploss_rel_backward(int batch, size_t n, const float* pred, const float* target, const float* stdv,
                                       int stat_len, float eps, const float* grad_loss, float* dpred, const void* ws,
                                       size_t ws_bytes, void* stream) {
  if (batch < 1 || n < 1 || !pred || !target || !dpred || !ws) return fail(FNO_EINVAL, "fno_lploss_rel_backward: bad argument");
  if (stdv && stat_len != 1 && (size_t)stat_len != n)
    return fail(FNO_EINVAL, "decode statistics must have 1 or %zu elements, got %d", n, stat_len);
  if (ws_bytes < fno_lploss_workspace_bytes(batch)) return fail(FNO_ENOMEM, "workspace too small");
  const float* coef = (const float*)ws + (size_t)batch * kLossSplit * 2;
  const int gx = (int)std::min<size_t>((n + 1023) / 1024, 64);
  LAUNCHCHK(launch("k_lploss_grad", k_lploss_grad, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, pred, target, stdv,
                   stat_len, eps, n, coef, grad_loss, dpred));
  return FNO_OK;
}
// Hyperparameters arrive as DOUBLES (the Python floats torch.optim.Adam holds): the step size, the bias corrections and the
// two (1 - beta) weights are formed in double and rounded once, as torch's scalar arguments are.
struct AdamHyper { float lr, beta1, beta2, eps, wd, omb1, omb2; };
static AdamHyper adam_hyper(double lr, double beta1, double beta2, double eps, double wd) {
  AdamHyper h;
  h.lr = (float)lr; h.beta1 = (float)beta1; h.beta2 = (float)beta2; h.eps = (float)eps; h.wd = (float)wd;
  h.omb1 = (float)(1.0 - beta1); h.omb2 = (float)(1.0 - beta2);
  return h;
}
extern "C" void fno_adam_scalars(double lr, double beta1, double beta2, int step, float* out2) {
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  out2[0] = (float)(lr / bc1);
  out2[1] = (float)std::sqrt(bc2);
}
extern "C" int fno_adam_prep_dev(int* step_counter, float* scratch2, double lr, double beta1, double beta2, void* stream) {
  if (!step_counter || !scratch2) return fail(FNO_EINVAL, "fno_adam_prep_dev: null step counter / scratch");
  return launch("k_adam_prep", k_adam_prep, dim3(1), dim3(1), 0, (hipStream_t)stream, step_counter, scratch2, lr, beta1, beta2);
}
extern "C" int fno_adam_step_range(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                                   double beta1, double beta2, double eps, double weight_decay, int step, const float* dyn,
                                   void* stream) {
  if (!n) return FNO_OK;
  if (!dyn && step < 1) return fail(FNO_EINVAL, "fno_adam_step: step must be >= 1 (or pass the prepared scalars)");
  if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(FNO_EINVAL, "fno_adam_step: bad argument");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
    return fail(FNO_EINVAL, "fno_adam_step: buffers must be 16-byte aligned");
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay);
  AdamArgs a;
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
  a.lr = h.lr; a.beta1 = h.beta1; a.beta2 = h.beta2; a.eps = h.eps; a.wd = h.wd; a.omb1 = h.omb1; a.omb2 = h.omb2;
  a.dyn = dyn; a.step_size = 0.f; a.bc2_sqrt = 1.f;
  if (!dyn) { float sc[2]; fno_adam_scalars(lr, beta1, beta2, step, sc); a.step_size = sc[0]; a.bc2_sqrt = sc[1]; }
  const int grid = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, (size_t)dev_ncu() * 8);
  return launch("k_adam", k_adam, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
}
extern "C" int fno_adam_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                             double beta1, double beta2, double eps, double weight_decay, int step, void* stream) {
  if (step < 1) return fail(FNO_EINVAL, "fno_adam_step: step must be >= 1");
  return fno_adam_step_range(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, nullptr, stream);
}
extern "C" int fno_adam_step_dev(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int* step_counter,
                                 float* scratch2, void* stream) {
  if (!n) return FNO_OK;
  LAUNCHCHK(fno_adam_prep_dev(step_counter, scratch2, lr, beta1, beta2, stream));
  return fno_adam_step_range(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, 0, scratch2, stream);
}
// ---- the same update on a bucket whose dialect-C weights are sliced (dead last-dim slices skipped and replayed later) ----
static int rows_check(const char* who, size_t rows, int row_len, int live_len) {
  if (!rows || row_len < 2 || live_len < 2 || live_len >= row_len || (row_len & 1) || (live_len & 1))
    return fail(FNO_EINVAL, "%s: need rows >= 1 and even 2 <= live_len < row_len (got %zu, %d, %d)", who, rows, live_len, row_len);
  return FNO_OK;
}
extern "C" int fno_adam_step_live(size_t rows, int row_len, int live_len, float* param, const float* grad, float* exp_avg_live,
                                  float* exp_avg_sq_live, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  int step, const float* dyn, void* stream) {
  LAUNCHCHK(rows_check("fno_adam_step_live", rows, row_len, live_len));
  if (!dyn && step < 1) return fail(FNO_EINVAL, "fno_adam_step_live: step must be >= 1 (or pass the prepared scalars)");
  if (!param || !grad || !exp_avg_live || !exp_avg_sq_live) return fail(FNO_EINVAL, "fno_adam_step_live: bad argument");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg_live | (uintptr_t)exp_avg_sq_live) & 7)
    return fail(FNO_EINVAL, "fno_adam_step_live: buffers must be 8-byte aligned");
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay);
  AdamLiveArgs a;
  a.p = param; a.g = grad; a.m = exp_avg_live; a.v = exp_avg_sq_live; a.rows = rows; a.row_len = row_len; a.live_len = live_len;
  a.beta1 = h.beta1; a.beta2 = h.beta2; a.eps = h.eps; a.wd = h.wd; a.omb1 = h.omb1; a.omb2 = h.omb2;
  a.dyn = dyn; a.step_size = 0.f; a.bc2_sqrt = 1.f;
  if (!dyn) { float sc[2]; fno_adam_scalars(lr, beta1, beta2, step, sc); a.step_size = sc[0]; a.bc2_sqrt = sc[1]; }
  const size_t n2 = rows * (size_t)(live_len / 2);
  const int grid = (int)std::min<size_t>((n2 + 255) / 256, (size_t)dev_ncu() * 8);
  return launch("k_adam_live", k_adam_live, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
}
extern "C" int fno_adam_replay_prep(float* scal, int step_from, int nsteps, double lr, double beta1, double beta2, void* stream) {
  if (!scal || step_from < 1 || nsteps < 1) return fail(FNO_EINVAL, "fno_adam_replay_prep: bad argument");
  return launch("k_adam_replay_prep", k_adam_replay_prep, dim3(std::min(64, (nsteps + 255) / 256)), dim3(256), 0,
                (hipStream_t)stream, scal, step_from, nsteps, lr, beta1, beta2);
}
extern "C" int fno_adam_replay_dead(size_t rows, int row_len, int live_len, float* param, float* dead_exp_avg,
                                    float* dead_exp_avg_sq, int moments_zero, const float* scal, int nsteps, double beta1,
                                    double beta2, double eps, double weight_decay, void* stream) {
  LAUNCHCHK(rows_check("fno_adam_replay_dead", rows, row_len, live_len));
  if (!param || !dead_exp_avg || !dead_exp_avg_sq || !scal || nsteps < 1)
    return fail(FNO_EINVAL, "fno_adam_replay_dead: bad argument");
  const AdamHyper h = adam_hyper(0.0, beta1, beta2, eps, weight_decay);
  AdamReplayArgs a;
  a.p = param; a.dm = dead_exp_avg; a.dv = dead_exp_avg_sq; a.rows = rows; a.row_len = row_len; a.live_len = live_len;
  a.moments_zero = moments_zero; a.scal = scal; a.nsteps = nsteps; a.beta1 = h.beta1; a.beta2 = h.beta2; a.eps = h.eps;
  a.wd = h.wd; a.omb1 = h.omb1; a.omb2 = h.omb2;
  const size_t n = rows * (size_t)(row_len - live_len);
  const int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)dev_ncu() * 16);
  return launch("k_adam_replay_dead", k_adam_replay_dead, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
}

// ===========================================================================
// PINO residual loss (spectral Navier-Stokes vorticity residual + initial-condition term)
// ===========================================================================
static const int kIcSplit = 16;
static const int kPinoChunk = 64;        // planes per pass of the slab kernels (bounds S1 / S2)
static int g_pino_twopass = 0;           // debug: route 128 x 128 planes through the slab kernels too (self-check vs the in-LDS path)
extern "C" void fno_debug_pino_twopass(int on) { g_pino_twopass = on ? 1 : 0; }
static bool pino_slabs(int n) { return n == 256 || (n == 128 && g_pino_twopass); }
struct PinoWs { float *fields, *dws, *part_f, *part_ic, *coef_f, *coef_ic; float2 *s1, *s2; int pp, chunk; size_t total; bool ok; };
static PinoWs carve_pino(int B, int n, int T, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  const size_t np = (size_t)B * (T - 2) * n * n;
  PinoWs w;
  w.pp = pino_slabs(n) ? n / PINO2_RB : 1;
  w.chunk = std::min(B * (T - 2), kPinoChunk);
  w.fields = c.take<float>(5 * np);
  w.dws = c.take<float>(np);
  w.part_f = c.take<float>((size_t)B * (T - 2) * w.pp);
  w.part_ic = c.take<float>((size_t)B * kIcSplit * 2);
  w.coef_f = c.take<float>(B);
  w.coef_ic = c.take<float>(B);
  w.s1 = w.s2 = nullptr;
  if (pino_slabs(n)) {
    w.s1 = c.take<float2>((size_t)w.chunk * n * n);
    w.s2 = c.take<float2>((size_t)5 * w.chunk * n * n);
  }
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
static int pino_check(int B, int n, int T) {
  if (B < 1 || T < 3) return fail(FNO_EINVAL, "pino loss: batch %d, %d time levels (need >= 3)", B, T);
  if (n != 32 && n != 64 && n != 128 && n != 256)
    return fail(FNO_EUNSUPPORTED, "pino loss: square grids of 32, 64, 128 or 256 points per side (got %d)", n);
  return FNO_OK;
}
extern "C" size_t fno_pino_loss_workspace_bytes(int batch, int n, int nt) {
  if (batch < 1 || n < 1 || nt < 3) return 0;
  return carve_pino(batch, n, nt, nullptr, 0).total;
}
template <int N>
static int pino_launch_planes(bool backward, int planes, hipStream_t st, const PinoArgs& a) {
  const size_t lds = ((size_t)N * (N + 1) + N / 2) * 8 + 64;
  if (backward) return launch("k_pino_plane_bwd", k_pino_plane_bwd<N>, dim3(planes), dim3(PinoCfg<N>::NT), lds, st, a);
  return launch("k_pino_plane_fwd", k_pino_plane_fwd<N>, dim3(planes), dim3(PinoCfg<N>::NT), lds, st, a);
}
// planes too large for one CU's LDS: row / column / row slab passes through HBM (k_pino_loss2.h), `chunk` planes at a time
template <int N>
static int pino_launch_slabs(bool backward, int planes, hipStream_t st, const PinoArgs& a, const PinoWs& w) {
  const size_t lds_r = ((size_t)PINO2_RB * (N + 1) + N / 2) * 8 + 64;
  const size_t lds_c = ((size_t)N * (PINO2_RB + 1) + N / 2) * 8;
  for (int p0 = 0; p0 < planes; p0 += w.chunk) {
    const int pc = std::min(w.chunk, planes - p0);
    Pino2Args b;
    b.p = a; b.s1 = w.s1; b.s2 = w.s2; b.plane0 = p0;
    const dim3 grid(N / PINO2_RB, pc), blk(PINO2_NT);
    if (!backward) {
      LAUNCHCHK(launch("k_pino2_rows_fwd", k_pino2_rows_fwd<N>, grid, blk, lds_r, st, b));
      LAUNCHCHK(launch("k_pino2_cols_fwd", k_pino2_cols_fwd<N>, grid, blk, lds_c, st, b));
      LAUNCHCHK(launch("k_pino2_rows_inv", k_pino2_rows_inv<N>, grid, blk, lds_r, st, b));
    } else {
      LAUNCHCHK(launch("k_pino2_rows_bwd", k_pino2_rows_bwd<N>, grid, blk, lds_r, st, b));
      LAUNCHCHK(launch("k_pino2_cols_bwd", k_pino2_cols_bwd<N>, grid, blk, lds_c, st, b));
      LAUNCHCHK(launch("k_pino2_rows_out", k_pino2_rows_out<N>, grid, blk, lds_r, st, b));
    }
  }
  return FNO_OK;
}
static int pino_planes(bool backward, int n, int planes, hipStream_t st, const PinoArgs& a, const PinoWs& w) {
  if (n == 32) return pino_launch_planes<32>(backward, planes, st, a);
  if (n == 64) return pino_launch_planes<64>(backward, planes, st, a);
  if (n == 256) return pino_launch_slabs<256>(backward, planes, st, a, w);
  if (pino_slabs(n)) return pino_launch_slabs<128>(backward, planes, st, a, w);
  return pino_launch_planes<128>(backward, planes, st, a);
}
extern "C" int fno_pino_loss_forward(int B, int n, int T, const float* u, const float* u0, const float* forcing,
                                     const float* visc, float t_interval, float* loss_ic, float* loss_f, void* ws,
                                     size_t ws_bytes, void* stream) {
  LAUNCHCHK(pino_check(B, n, T));
  if (!u || !u0 || !forcing || !visc || !loss_ic || !loss_f || !ws) return fail(FNO_EINVAL, "fno_pino_loss_forward: null argument");
  PinoWs w = carve_pino(B, n, T, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  PinoArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.forcing = forcing; a.visc = visc; a.fields = w.fields; a.partial = w.part_f;
  a.B = B; a.T = T; a.inv2dt = (float)((double)(T - 1) / (2.0 * (double)t_interval));
  LAUNCHCHK(pino_planes(false, n, B * (T - 2), st, a, w));
  LAUNCHCHK(launch("k_pino_ic_partial", k_pino_ic_partial, dim3(kIcSplit, B), dim3(256), 0, st, u, u0, n * n, T, w.part_ic));
  LAUNCHCHK(launch("k_pino_finish", k_pino_finish, dim3(1), dim3(256), 0, st, (const float*)w.part_f, (const float*)w.part_ic,
                   forcing, B, T, n * n, kIcSplit, w.pp, loss_ic, loss_f, w.coef_ic, w.coef_f));
  return FNO_OK;
}
extern "C" int fno_pino_loss_backward(int B, int n, int T, const float* u, const float* u0, const float* forcing,
                                      const float* visc, float t_interval, const float* g_ic, const float* g_f, float* du,
                                      void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(pino_check(B, n, T));
  if (!u || !u0 || !visc || !du || !ws) return fail(FNO_EINVAL, "fno_pino_loss_backward: null argument");
  PinoWs w = carve_pino(B, n, T, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  const size_t np = (size_t)B * (T - 2) * n * n;
  PinoArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.forcing = forcing; a.visc = visc; a.fields = w.fields; a.dws = w.dws; a.coef_f = w.coef_f; a.g_f = g_f;
  a.B = B; a.T = T; a.inv2dt = (float)((double)(T - 1) / (2.0 * (double)t_interval));
  LAUNCHCHK(pino_planes(true, n, B * (T - 2), st, a, w));
  const size_t npix = (size_t)B * n * n;
  LAUNCHCHK(launch("k_pino_assemble", k_pino_assemble, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, u, u0,
                   (const float*)w.dws, (const float*)(w.fields + 4 * np), (const float*)w.coef_f, (const float*)w.coef_ic,
                   g_f, g_ic, B, n * n, T, a.inv2dt, du));
  return FNO_OK;
}

// ===========================================================================
// Burgers residual loss (k_burgers_loss.h): FDM_Burgers + PINO_loss, libs/pino_utils/losses.py:200-243
// ===========================================================================
static int burgers_check(int B, int nt, int nx) {
  if (B < 1) return fail(FNO_EINVAL, "burgers loss: batch=%d (at least 1)", B);
  if (nt < 3) return fail(FNO_EINVAL, "burgers loss: nt=%d (at least 3 time rows: one interior row)", nt);
  if (nx < 2 || (nx & 1)) return fail(FNO_EINVAL, "burgers loss: nx=%d (even: the wavenumber table has 2 (nx / 2) entries)", nx);
  if (nx != 32 && nx != 64 && nx != 128)
    return fail(FNO_EUNSUPPORTED, "burgers loss: nx=%d (rows of 32, 64 or 128 points)", nx);
  if ((size_t)B * (size_t)((nt + BURG_TJ - 1) / BURG_TJ) > 0x7fffffffull)
    return fail(FNO_EUNSUPPORTED, "burgers loss: batch=%d times nt=%d exceeds the grid limit", B, nt);
  return FNO_OK;
}
static int burgers_tiles_fwd(int nt) { return (nt - 2 + BURG_TJ - 1) / BURG_TJ; }
static int burgers_tiles_bwd(int nt) { return (nt + BURG_TJ - 1) / BURG_TJ; }
struct BurgersWs { float *Du, *ux; double *part_f, *part_u; size_t total; bool ok; };
static BurgersWs carve_burgers(int B, int nt, int nx, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  const size_t np = (size_t)B * (nt - 2) * nx;
  BurgersWs w;
  w.Du = c.take<float>(np);
  w.ux = c.take<float>(np);
  w.part_f = c.take<double>((size_t)B * burgers_tiles_fwd(nt));
  w.part_u = c.take<double>(B);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
extern "C" size_t fno_burgers_loss_workspace_bytes(int batch, int nt, int nx) {
  if (batch < 1 || nt < 3 || nx < 1) return 0;
  return carve_burgers(batch, nt, nx, nullptr, 0).total;
}
static BurgersArgs burgers_args(int B, int nt, int nx, const float* u, const float* u0, float visc, const BurgersWs& w) {
  BurgersArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.u0 = u0; a.Du = w.Du; a.ux = w.ux; a.part_f = w.part_f; a.part_u = w.part_u;
  a.B = B; a.nt = nt; a.visc = visc;
  a.inv2dt = (float)((double)(nt - 1) / 2.0);
  a.scale_f = (float)(2.0 / ((double)B * (nt - 2) * nx));
  a.scale_u = (float)(2.0 / ((double)B * nx));
  return a;
}
extern "C" int fno_burgers_loss_forward(int B, int nt, int nx, const float* u, const float* u0, float visc, float* loss_u,
                                        float* loss_f, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(burgers_check(B, nt, nx));
  if (!u || !u0 || !loss_u || !loss_f || !ws) return fail(FNO_EINVAL, "fno_burgers_loss_forward: null argument");
  BurgersWs w = carve_burgers(B, nt, nx, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  BurgersArgs a = burgers_args(B, nt, nx, u, u0, visc, w);
  a.tiles = burgers_tiles_fwd(nt);
  const dim3 grid((unsigned)(B * a.tiles)), blk(BURG_NT);
  if (nx == 32) LAUNCHCHK(launch("k_burgers_fwd", k_burgers_fwd<32>, grid, blk, 0, st, a));
  else if (nx == 64) LAUNCHCHK(launch("k_burgers_fwd", k_burgers_fwd<64>, grid, blk, 0, st, a));
  else LAUNCHCHK(launch("k_burgers_fwd", k_burgers_fwd<128>, grid, blk, 0, st, a));
  return launch("k_burgers_finish", k_burgers_finish, dim3(1), dim3(256), 0, st, (const double*)w.part_f, B * a.tiles,
                (const double*)w.part_u, B, 1.0 / ((double)B * (nt - 2) * nx), 1.0 / ((double)B * nx), loss_u, loss_f);
}
extern "C" int fno_burgers_loss_backward(int B, int nt, int nx, const float* u, const float* u0, float visc, const float* g_u,
                                         const float* g_f, float* du, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(burgers_check(B, nt, nx));
  if (!u || !u0 || !du || !ws) return fail(FNO_EINVAL, "fno_burgers_loss_backward: null argument");
  BurgersWs w = carve_burgers(B, nt, nx, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  BurgersArgs a = burgers_args(B, nt, nx, u, u0, visc, w);
  a.g_u = g_u; a.g_f = g_f; a.du = du;
  a.tiles = burgers_tiles_bwd(nt);
  const dim3 grid((unsigned)(B * a.tiles)), blk(BURG_NT);
  hipStream_t st = (hipStream_t)stream;
  if (nx == 32) return launch("k_burgers_bwd", k_burgers_bwd<32>, grid, blk, 0, st, a);
  if (nx == 64) return launch("k_burgers_bwd", k_burgers_bwd<64>, grid, blk, 0, st, a);
  return launch("k_burgers_bwd", k_burgers_bwd<128>, grid, blk, 0, st, a);
}

// ===========================================================================
// Darcy residual loss (k_darcy_loss.h): FDM_Darcy + darcy_loss, libs/pino_utils/losses.py:6-65, with the mollifier and the
// relative-L2 data term of train_2d.py:58-82
// ===========================================================================
static int darcy_tiles(int S) { return (S - 4 + DARCY_T - 1) / DARCY_T; }
static int darcy_check(int B, int S) {
  if (B < 1) return fail(FNO_EINVAL, "darcy loss: batch=%d (at least 1)", B);
  if (S < 5) return fail(FNO_EINVAL, "darcy loss: S=%d (at least 5 points a side: one residual cell)", S);
  if (S > DARCY_SMAX) return fail(FNO_EUNSUPPORTED, "darcy loss: S=%d (at most %d points a side)", S, DARCY_SMAX);
  if ((size_t)B * (size_t)darcy_tiles(S) * (size_t)darcy_tiles(S) > 0x7fffffffull)
    return fail(FNO_EUNSUPPORTED, "darcy loss: batch=%d times S=%d exceeds the grid limit", B, S);
  return FNO_OK;
}
struct DarcyWs { float* Du; double *part, *norms; size_t total; bool ok; };
static DarcyWs carve_darcy(int B, int S, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  DarcyWs w;
  w.Du = c.take<float>((size_t)B * (S - 4) * (S - 4));
  w.part = c.take<double>((size_t)B * darcy_tiles(S) * darcy_tiles(S) * 3);
  w.norms = c.take<double>((size_t)B * 3);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
extern "C" size_t fno_darcy_loss_workspace_bytes(int batch, int S) {
  if (batch < 1 || S < 5 || S > DARCY_SMAX) return 0;
  return carve_darcy(batch, S, nullptr, 0).total;
}
static DarcyArgs darcy_args(int B, int S, const float* out, const float* mol, const float* a, const float* y, const DarcyWs& w) {
  DarcyArgs d;
  memset(&d, 0, sizeof(d));
  d.out = out; d.mol = mol; d.a = a; d.y = y; d.Du = w.Du; d.part = w.part; d.norms = w.norms;
  d.B = B; d.S = S; d.tiles = darcy_tiles(S);
  d.inv4h2 = (float)((double)(S - 1) * (double)(S - 1) / 4.0);
  return d;
}
extern "C" int fno_darcy_loss_forward(int B, int S, const float* out, const float* mol, const float* a, const float* y,
                                      float* loss_data, float* loss_f, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(darcy_check(B, S));
  if ((y != nullptr) != (loss_data != nullptr))
    return fail(FNO_EINVAL, "fno_darcy_loss_forward: y=%p and loss_data=%p (both or neither: the data term needs its target and its "
                "result)", (const void*)y, (void*)loss_data);
  if (!out || !a || !loss_f || !ws) return fail(FNO_EINVAL, "fno_darcy_loss_forward: null argument");
  DarcyWs w = carve_darcy(B, S, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  DarcyArgs d = darcy_args(B, S, out, mol, a, y, w);
  const int per = d.tiles * d.tiles;
  LAUNCHCHK(launch("k_darcy_fwd", k_darcy_fwd, dim3((unsigned)(B * per)), dim3(DARCY_NT), 0, st, d));
  return launch("k_darcy_finish", k_darcy_finish, dim3(1), dim3(256), 0, st, (const double*)w.part, B, per, S, w.norms, loss_data,
                loss_f);
}
extern "C" int fno_darcy_loss_backward(int B, int S, const float* out, const float* mol, const float* a, const float* y,
                                       const float* g_data, const float* g_f, float* dout, void* ws, size_t ws_bytes,
                                       void* stream) {
  LAUNCHCHK(darcy_check(B, S));
  if (!out || !a || !dout || !ws) return fail(FNO_EINVAL, "fno_darcy_loss_backward: null argument");
  DarcyWs w = carve_darcy(B, S, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  DarcyArgs d = darcy_args(B, S, out, mol, a, y, w);
  d.g_data = g_data; d.g_f = g_f; d.dout = dout;
  return launch("k_darcy_bwd", k_darcy_bwd, dim3((unsigned)(B * d.tiles * d.tiles)), dim3(DARCY_NT), 0, (hipStream_t)stream, d);
}

// ===========================================================================
// Sobolev (H1) and L2 training losses of neuralop (k_sobolev_loss.h): LpLoss (p = 2) and H1Loss, neuralop/training/losses.py:62-277
// ===========================================================================
struct SobGeom { int D, n[3], c[3], per, seg; size_t plane; };
static int sob_check(int planes, int channels, int d, const int* dims, int order, int relative, int fix_mask, int batch_reduce,
                     SobGeom* out) {
  if (d < 1 || d > 3) return fail(FNO_EINVAL, "sobolev loss: d=%d (1, 2 or 3 grid axes)", d);
  if (!dims) return fail(FNO_EINVAL, "sobolev loss: dims is null");
  for (int k = 0; k < d; ++k)
    if (dims[k] < 2) return fail(FNO_EINVAL, "sobolev loss: extent %d of grid axis %d (at least 2)", dims[k], k);
  if (planes < 1) return fail(FNO_EINVAL, "sobolev loss: planes=%d (at least 1)", planes);
  if (order != 0 && order != 1) return fail(FNO_EINVAL, "sobolev loss: order=%d (0: Lp, 1: H1)", order);
  if (relative != 0 && relative != 1) return fail(FNO_EINVAL, "sobolev loss: relative=%d (0 or 1)", relative);
  if (fix_mask < 0 || fix_mask >= (1 << d)) return fail(FNO_EINVAL, "sobolev loss: fix_mask=%d (one bit per grid axis, d=%d)", fix_mask, d);
  if (batch_reduce != SOB_REDUCE_NONE && batch_reduce != SOB_REDUCE_SUM && batch_reduce != SOB_REDUCE_MEAN)
    return fail(FNO_EINVAL, "sobolev loss: batch_reduce=%d (0 none, 1 sum, 2 mean)", batch_reduce);
  if (batch_reduce != SOB_REDUCE_NONE && (channels < 1 || planes % channels != 0))
    return fail(FNO_EINVAL, "sobolev loss: channels=%d does not divide planes=%d (the batch reduction takes a (B, C) layout)", channels,
                planes);
  SobGeom g;
  g.plane = 1;
  for (int k = 0; k < d; ++k) g.plane *= (size_t)dims[k];
  if (g.plane >= 0x80000000ull)
    return fail(FNO_EUNSUPPORTED, "sobolev loss: a plane of %zu elements (fewer than 2^31)", g.plane);
  g.D = order ? d : 1;
  for (int k = 0; k < 3; ++k) { g.n[k] = 1; g.c[k] = 1; }
  if (order) {
    for (int k = 0; k < d; ++k) g.n[3 - d + k] = dims[k];
    const int t[3] = {d == 3 ? SOB_T3D_Z : 1, d == 3 ? SOB_T3D_Y : d == 2 ? SOB_T2D_Y : 1,
                      d == 3 ? SOB_T3D_X : d == 2 ? SOB_T2D_X : SOB_T1D_X};
    for (int k = 0; k < 3; ++k) g.c[k] = (g.n[k] + t[k] - 1) / t[k];
  } else {
    g.n[2] = (int)g.plane;
    g.c[2] = (g.n[2] + SOB_T0 - 1) / SOB_T0;
  }
  const size_t per = (size_t)g.c[0] * g.c[1] * g.c[2];
  if (per * (size_t)planes > 0x7fffffffull)
    return fail(FNO_EUNSUPPORTED, "sobolev loss: planes=%d times %zu tiles exceeds the grid limit", planes, per);
  g.per = (int)per;
  g.seg = 1;
  while (g.seg < g.per && g.seg < 64) g.seg <<= 1;
  if (out) *out = g;
  return FNO_OK;
}
struct SobWs { double *part, *stats; size_t total; bool ok; };
static SobWs carve_sobolev(int planes, const SobGeom& g, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  SobWs w;
  w.part = c.take<double>((size_t)planes * g.per * 2);
  w.stats = c.take<double>((size_t)planes * 2);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
extern "C" size_t fno_sobolev_loss_workspace_bytes(int planes, int d, const int* dims, int order) {
  SobGeom g;
  if (sob_check(planes, 1, d, dims, order, 0, 0, SOB_REDUCE_NONE, &g) != FNO_OK) return 0;
  return carve_sobolev(planes, g, nullptr, 0).total;
}
static SobolevArgs sobolev_args(const SobGeom& g, int planes, int channels, int d, int relative, int fix_mask, int batch_reduce,
                                const double* inv2h, const double* invh, double vol, const float* x, const float* y,
                                const SobWs& w) {
  SobolevArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.part = w.part; a.stats = w.stats;
  for (int k = 0; k < 3; ++k) { a.n[k] = g.n[k]; a.c[k] = g.c[k]; a.inv2h[k] = 0.f; a.invh[k] = 0.f; }
  for (int k = 0; k < d; ++k) {
    a.fix[3 - d + k] = (fix_mask >> k) & 1;
    a.inv2h[3 - d + k] = (float)inv2h[k];
    a.invh[3 - d + k] = (float)invh[k];
  }
  a.per = g.per;
  a.relative = relative; a.reduce = batch_reduce;
  a.channels = batch_reduce == SOB_REDUCE_NONE ? 1 : channels;
  a.batch = batch_reduce == SOB_REDUCE_NONE ? 1 : planes / channels;
  a.vol = vol;
  return a;
}
extern "C" int fno_sobolev_loss_forward(int planes, int channels, int d, const int* dims, int order, int relative, int fix_mask,
                                        int batch_reduce, const double* inv2h, const double* invh, double vol, const float* x,
                                        const float* y, float* value, float* reduced, void* ws, size_t ws_bytes, void* stream) {
  SobGeom g;
  LAUNCHCHK(sob_check(planes, channels, d, dims, order, relative, fix_mask, batch_reduce, &g));
  if (!x || !y || !value || !ws || !inv2h || !invh || (batch_reduce != SOB_REDUCE_NONE && !reduced))
    return fail(FNO_EINVAL, "fno_sobolev_loss_forward: null argument");
  SobWs w = carve_sobolev(planes, g, ws, ws_bytes);
  if (!w.ok) return fail(FNO_EINVAL, "fno_sobolev_loss_forward: workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  SobolevArgs a = sobolev_args(g, planes, channels, d, relative, fix_mask, batch_reduce, inv2h, invh, vol, x, y, w);
  const dim3 grid((unsigned)((size_t)planes * g.per)), blk(SOB_NT);
  if (!order) LAUNCHCHK(launch("k_sobolev_fwd", k_sobolev_fwd<1, 0>, grid, blk, 0, st, a));
  else if (d == 1) LAUNCHCHK(launch("k_sobolev_fwd", k_sobolev_fwd<1, 1>, grid, blk, 0, st, a));
  else if (d == 2) LAUNCHCHK(launch("k_sobolev_fwd", k_sobolev_fwd<2, 1>, grid, blk, 0, st, a));
  else LAUNCHCHK(launch("k_sobolev_fwd", k_sobolev_fwd<3, 1>, grid, blk, 0, st, a));
  SobolevFinish f;
  memset(&f, 0, sizeof(f));
  f.part = w.part; f.stats = w.stats; f.value = value; f.reduced = reduced;
  f.planes = planes; f.per = g.per; f.seg = g.seg;
  f.relative = relative; f.reduce = batch_reduce; f.batch = a.batch; f.vol = vol;
  const int nseg = SOB_NT / g.seg;
  unsigned groups;
  if (batch_reduce == SOB_REDUCE_NONE) { f.cnt = nseg; f.gstride = nseg; f.jstride = 1; groups = (unsigned)((planes + nseg - 1) / nseg); }
  else { f.cnt = a.batch; f.gstride = 1; f.jstride = channels; groups = (unsigned)channels; }
  return launch("k_sobolev_finish", k_sobolev_finish, dim3(groups), blk, 0, st, f);
}
extern "C" int fno_sobolev_loss_backward(int planes, int channels, int d, const int* dims, int order, int relative, int fix_mask,
                                         int batch_reduce, const double* inv2h, const double* invh, double vol, const float* x,
                                         const float* y, const float* grad, float* dx, void* ws, size_t ws_bytes, void* stream) {
  SobGeom g;
  LAUNCHCHK(sob_check(planes, channels, d, dims, order, relative, fix_mask, batch_reduce, &g));
  if (!x || !y || !grad || !dx || !ws || !inv2h || !invh) return fail(FNO_EINVAL, "fno_sobolev_loss_backward: null argument");
  SobWs w = carve_sobolev(planes, g, ws, ws_bytes);
  if (!w.ok) return fail(FNO_EINVAL, "fno_sobolev_loss_backward: workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  SobolevArgs a = sobolev_args(g, planes, channels, d, relative, fix_mask, batch_reduce, inv2h, invh, vol, x, y, w);
  a.grad = grad; a.dx = dx;
  const dim3 grid((unsigned)((size_t)planes * g.per)), blk(SOB_NT);
  if (!order) return launch("k_sobolev_bwd", k_sobolev_bwd<1, 0>, grid, blk, 0, st, a);
  if (d == 1) return launch("k_sobolev_bwd", k_sobolev_bwd<1, 1>, grid, blk, 0, st, a);
  if (d == 2) return launch("k_sobolev_bwd", k_sobolev_bwd<2, 1>, grid, blk, 0, st, a);
  return launch("k_sobolev_bwd", k_sobolev_bwd<3, 1>, grid, blk, 0, st, a);
}

// ===========================================================================
// Spectral Sobolev loss of the original FNO code base (k_hs_loss.h): HsLoss, libs/utilities3.py:339-405
// ===========================================================================
static int hs_slots(int channels) { return (channels + 1) / 2; }      // a workgroup takes a pair of channels as one complex plane
static int hs_check(int B, int nx, int ny, int C, int terms, const double* w2, int group, double divisor, int reduce) {
  if (nx != ny) return fail(FNO_EINVAL, "hs loss: a %d x %d plane (square planes of 32, 64 or 128 points a side)", nx, ny);
  if (nx != 32 && nx != 64 && nx != 128)
    return fail(FNO_EINVAL, "hs loss: a %d x %d plane (square planes of 32, 64 or 128 points a side)", nx, ny);
  if (B < 1) return fail(FNO_EINVAL, "hs loss: batch=%d (at least 1)", B);
  if (C < 1) return fail(FNO_EINVAL, "hs loss: channels=%d (at least 1)", C);
  if (terms < 1 || terms > HS_TERMS) return fail(FNO_EINVAL, "hs loss: terms=%d (1 to %d: |k|^0, |k|^2, |k|^4)", terms, HS_TERMS);
  if (!w2) return fail(FNO_EINVAL, "hs loss: w2 is null");
  if (group != 0 && group != 1) return fail(FNO_EINVAL, "hs loss: group=%d (0 or 1)", group);
  if (group && !(divisor > 0.0)) return fail(FNO_EINVAL, "hs loss: divisor=%g of the grouped form (positive: k + 1)", divisor);
  if (reduce != HS_REDUCE_NONE && reduce != HS_REDUCE_SUM && reduce != HS_REDUCE_MEAN)
    return fail(FNO_EINVAL, "hs loss: reduce=%d (0 none, 1 sum, 2 mean)", reduce);
  if ((size_t)B * (size_t)hs_slots(C) > 0x7fffffffull)
    return fail(FNO_EUNSUPPORTED, "hs loss: batch=%d times %d channel pairs exceeds the grid limit", B, hs_slots(C));
  return FNO_OK;
}
struct HsWs { double *part, *stats; size_t total; bool ok; };
static HsWs carve_hs(int B, int C, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  HsWs w;
  w.part = c.take<double>((size_t)B * hs_slots(C) * 2 * HS_TERMS);
  w.stats = c.take<double>((size_t)B * 2 * HS_TERMS);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
extern "C" size_t fno_hs_loss_workspace_bytes(int batch, int channels) {
  if (batch < 1 || channels < 1 || (size_t)batch * (size_t)hs_slots(channels) > 0x7fffffffull) return 0;
  return carve_hs(batch, channels, nullptr, 0).total;
}
static HsArgs hs_args(int B, int C, int terms, const double* w2, int group, double divisor, int reduce, const float* x,
                      const float* y, const HsWs& w) {
  HsArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.part = w.part; a.stats = w.stats;
  a.C = C; a.slots = hs_slots(C); a.terms = terms; a.group = group; a.reduce = reduce; a.batch = B;
  for (int j = 0; j < terms; ++j) a.w2[j] = w2[j];
  a.divisor = group ? divisor : 1.0;
  return a;
}
template <int N>
static int hs_launch_planes(bool backward, hipStream_t st, const HsArgs& a) {
  const size_t lds = ((size_t)N * (N + 1) + N / 2) * 8 + (size_t)(PinoCfg<N>::NT / 64) * HS_TERMS * 8;
  const dim3 grid((unsigned)(a.batch * a.slots)), blk(PinoCfg<N>::NT);
  if (backward) return launch("k_hs_plane_bwd", k_hs_plane_bwd<N>, grid, blk, lds, st, a);
  return launch("k_hs_plane_fwd", k_hs_plane_fwd<N>, grid, blk, lds, st, a);
}
static int hs_planes(bool backward, int n, hipStream_t st, const HsArgs& a) {
  if (n == 32) return hs_launch_planes<32>(backward, st, a);
  if (n == 64) return hs_launch_planes<64>(backward, st, a);
  return hs_launch_planes<128>(backward, st, a);
}
extern "C" int fno_hs_loss_forward(int B, int nx, int ny, int C, int terms, const double* w2, int group, double divisor, int reduce,
                                   const float* x, const float* y, float* value, float* reduced, void* ws, size_t ws_bytes,
                                   void* stream) {
  LAUNCHCHK(hs_check(B, nx, ny, C, terms, w2, group, divisor, reduce));
  if (!x || !y || !value || !ws || (reduce != HS_REDUCE_NONE && !reduced)) return fail(FNO_EINVAL, "fno_hs_loss_forward: null argument");
  HsWs w = carve_hs(B, C, ws, ws_bytes);
  if (!w.ok) return fail(FNO_EINVAL, "fno_hs_loss_forward: workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  HsArgs a = hs_args(B, C, terms, w2, group, divisor, reduce, x, y, w);
  LAUNCHCHK(hs_planes(false, nx, st, a));
  HsFinish f;
  memset(&f, 0, sizeof(f));
  f.part = w.part; f.stats = w.stats; f.value = value; f.reduced = reduced;
  f.B = B; f.slots = a.slots; f.terms = terms; f.group = group; f.reduce = reduce; f.divisor = a.divisor;
  for (int j = 0; j < terms; ++j) f.w2[j] = w2[j];
  return launch("k_hs_finish", k_hs_finish, dim3(1), dim3(HS_FINISH_NT), 0, st, f);
}
extern "C" int fno_hs_loss_backward(int B, int nx, int ny, int C, int terms, const double* w2, int group, double divisor, int reduce,
                                    const float* x, const float* y, const float* grad, float* dx, void* ws, size_t ws_bytes,
                                    void* stream) {
  LAUNCHCHK(hs_check(B, nx, ny, C, terms, w2, group, divisor, reduce));
  if (!x || !y || !grad || !dx || !ws) return fail(FNO_EINVAL, "fno_hs_loss_backward: null argument");
  HsWs w = carve_hs(B, C, ws, ws_bytes);
  if (!w.ok) return fail(FNO_EINVAL, "fno_hs_loss_backward: workspace too small: need %zu, have %zu", w.total, ws_bytes);
  HsArgs a = hs_args(B, C, terms, w2, group, divisor, reduce, x, y, w);
  a.grad = grad; a.dx = dx;
  return hs_planes(true, nx, (hipStream_t)stream, a);
}

// ===========================================================================
// Channel-flow RHS + physics-informed loss (libs/envs/control_env.py:429-530, 627-633)
// ===========================================================================
extern "C" int fno_chanflow_pack_metrics(int Ny, const double* y, const double* ym, const double* yg, double* packed) {
  if (Ny < 3 || !y || !ym || !yg || !packed) return fail(FNO_EINVAL, "fno_chanflow_pack_metrics: Ny >= 3 and non-null arrays");
  const int MP = Ny + 2;
  for (int t = 0; t < 3 * MP; ++t) packed[t] = 0.0;
  for (int j = 1; j <= Ny - 1; ++j) packed[j] = 1.0 / (y[j] - y[j - 1]);
  for (int j = 1; j <= Ny - 2; ++j) packed[MP + j] = 1.0 / (ym[j] - ym[j - 1]);
  for (int j = 1; j <= Ny; ++j) packed[2 * MP + j] = 1.0 / (yg[j] - yg[j - 1]);
  for (int t = 0; t < 3 * MP; ++t)
    if (!std::isfinite(packed[t])) return fail(FNO_EINVAL, "fno_chanflow_pack_metrics: repeated grid point");
  return FNO_OK;
}
static int chanflow_geo(const FnoChanflowGrid* g, int B, const double* metrics, ChanflowGeo* out) {
  if (!g || !metrics) return fail(FNO_EINVAL, "chanflow: null grid or metrics");
  if (B < 1 || g->Nx < 2 || g->Ny < 3 || g->Nz < 2) return fail(FNO_EINVAL, "chanflow: need batch >= 1, Nx, Nz >= 2, Ny >= 3");
  if (!(g->dx > 0) || !(g->dz > 0)) return fail(FNO_EINVAL, "chanflow: dx and dz must be positive");
  if ((size_t)B * g->Nx > 0x7fffffffull) return fail(FNO_EINVAL, "chanflow: batch * Nx exceeds the grid limit");
  if ((size_t)(g->Ny + 1) * g->Nz > 0x3fffffffull) return fail(FNO_EINVAL, "chanflow: slab too large");
  out->B = B; out->Nx = g->Nx; out->Ny = g->Ny; out->Nz = g->Nz;
  out->rdx = 1.0 / g->dx; out->rdz = 1.0 / g->dz; out->nu = g->nu; out->metrics = metrics;
  return FNO_OK;
}
// slabs are split along y so that the launch carries ~8 waves per SIMD (one slab per workgroup leaves 4)
static int chanflow_ysplit(int B, int Nx) {
  const long wgs = (long)B * Nx, want = (long)dev_ncu() * 8;
  long s = (want + wgs - 1) / wgs;
  return (int)std::max(1L, std::min(s, 16L));
}
template <typename T>
static int chanflow_rhs_t(const ChanflowGeo& geo, const void* U, const void* V, const void* W, const void* dpdx,
                          double dpdx_default, void* Fu, void* Fv, void* Fw, hipStream_t st) {
  ChanflowRhsArgs<T> a;
  a.U = (const T*)U; a.V = (const T*)V; a.W = (const T*)W; a.dPdx = (const T*)dpdx;
  a.Fu = (T*)Fu; a.Fv = (T*)Fv; a.Fw = (T*)Fw; a.dPdx_default = (T)dpdx_default;
  return launch("k_chanflow_rhs", k_chanflow_rhs<T>, dim3((unsigned)(geo.B * geo.Nx), chanflow_ysplit(geo.B, geo.Nx)), dim3(256), 0, st, geo, a);
}
extern "C" int fno_chanflow_rhs(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const void* U,
                                const void* V, const void* W, const void* dpdx, double dpdx_default, void* Fu, void* Fv,
                                void* Fw, void* stream) {
  ChanflowGeo geo;
  LAUNCHCHK(chanflow_geo(grid, B, metrics, &geo));
  if (!U || !V || !W || !Fu || !Fv || !Fw) return fail(FNO_EINVAL, "fno_chanflow_rhs: null field");
  if (dtype == 0) return chanflow_rhs_t<float>(geo, U, V, W, dpdx, dpdx_default, Fu, Fv, Fw, (hipStream_t)stream);
  if (dtype == 1) return chanflow_rhs_t<double>(geo, U, V, W, dpdx, dpdx_default, Fu, Fv, Fw, (hipStream_t)stream);
  return fail(FNO_EINVAL, "fno_chanflow_rhs: dtype must be 0 (fp32) or 1 (fp64)");
}
struct ChanflowWs { float *Du, *Dv, *Dw, *partial, *inv_norm; size_t total; bool ok; };
static ChanflowWs carve_chanflow(const FnoChanflowGrid* g, int B, void* ws, size_t ws_bytes) {
  ChanflowWs w;
  const size_t su = (size_t)B * g->Nx * (g->Ny + 1) * g->Nz, sv = (size_t)B * g->Nx * g->Ny * g->Nz;
  auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
  float* p = (float*)ws;
  w.Du = p; p += up(su);
  w.Dw = p; p += up(su);
  w.Dv = p; p += up(sv);
  w.partial = p; p += up((size_t)B * g->Nx * 16 * 3);
  w.inv_norm = p; p += up((size_t)B * 3);
  w.total = (size_t)((char*)p - (char*)ws);
  w.ok = ws_bytes >= w.total;
  return w;
}
extern "C" size_t fno_chanflow_pde_loss_workspace_bytes(const FnoChanflowGrid* grid, int B) {
  if (!grid || B < 1 || grid->Nx < 1 || grid->Ny < 1 || grid->Nz < 1) return 0;
  return carve_chanflow(grid, B, nullptr, 0).total;
}
extern "C" int fno_chanflow_pde_loss_forward(const FnoChanflowGrid* grid, int B, const double* metrics, const float* U,
                                             const float* Vgt, const float* V, const float* W, float* loss, void* ws,
                                             size_t ws_bytes, void* stream) {
  ChanflowGeo geo;
  LAUNCHCHK(chanflow_geo(grid, B, metrics, &geo));
  if (!U || !Vgt || !V || !W || !loss || !ws) return fail(FNO_EINVAL, "fno_chanflow_pde_loss_forward: null argument");
  ChanflowWs w = carve_chanflow(grid, B, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  ChanflowLossArgs a;
  memset(&a, 0, sizeof(a));
  a.U = U; a.Vgt = Vgt; a.V = V; a.W = W; a.Du = w.Du; a.Dv = w.Dv; a.Dw = w.Dw; a.partial = w.partial;
  const int ys = chanflow_ysplit(B, grid->Nx);
  LAUNCHCHK(launch("k_chanflow_diff", k_chanflow_diff, dim3((unsigned)(B * grid->Nx), ys), dim3(256), 0, st, geo, a));
  LAUNCHCHK(launch("k_chanflow_finish", k_chanflow_finish, dim3(1), dim3(256), 0, st, B, grid->Nx * ys, (const float*)w.partial,
                   w.inv_norm, loss));
  return FNO_OK;
}
extern "C" int fno_chanflow_pde_loss_backward(const FnoChanflowGrid* grid, int B, const double* metrics, const float* U,
                                              const float* Vgt, const float* V, const float* W, const float* gloss, float* dV,
                                              void* ws, size_t ws_bytes, void* stream) {
  ChanflowGeo geo;
  LAUNCHCHK(chanflow_geo(grid, B, metrics, &geo));
  if (!U || !Vgt || !V || !W || !dV || !ws) return fail(FNO_EINVAL, "fno_chanflow_pde_loss_backward: null argument");
  ChanflowWs w = carve_chanflow(grid, B, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  ChanflowLossArgs a;
  memset(&a, 0, sizeof(a));
  a.U = U; a.Vgt = Vgt; a.V = V; a.W = W; a.Du = w.Du; a.Dv = w.Dv; a.Dw = w.Dw; a.inv_norm = w.inv_norm;
  a.gloss = gloss; a.dV = dV;
  return launch("k_chanflow_diff_bwd", k_chanflow_diff_bwd, dim3((unsigned)(B * grid->Nx), chanflow_ysplit(B, grid->Nx)), dim3(256), 0, (hipStream_t)stream,
                geo, a);
}

// ===========================================================================
// Channel-flow environment step, fp64 (libs/envs/control_env.py:533-613 RK3 + projection, :196-229 pressure, :186-303 scores)
// ===========================================================================
struct CfTabLayout { int twx, twz, wgt, trap, sub, fac, ntile; size_t total; };
static CfTabLayout cf_tab_layout(int Nx, int Ny, int Nz) {
  auto even = [](int n) { return (n + 1) & ~1; };
  CfTabLayout l;
  const int Nzh = Nz / 2 + 1, n = Ny - 1;
  l.twx = 0;
  l.twz = l.twx + 2 * Nx;
  l.wgt = l.twz + 2 * Nz;
  l.trap = l.wgt + even(Nzh);
  l.sub = l.trap + even(n);
  l.fac = l.sub + even(n);
  l.ntile = (Nx * Nzh + kCfTile - 1) / kCfTile;
  l.total = ((size_t)l.fac + (size_t)l.ntile * n * kCfTile * 2) * sizeof(double);
  return l;
}
// LDS of the transform kernels: spectrum plane + twiddles (+ c2r weights) + a chunk of `xc` (+ halo) real rows
static size_t cf_plane_lds(int Nx, int Nz, int xc, bool inverse) {
  const int Nzh = Nz / 2 + 1;
  size_t d = (size_t)Nx * Nzh * 2 + 2 * (size_t)(Nx + Nz);
  if (inverse) d += ((Nzh + 1) & ~1) + (size_t)(xc + 1) * (Nz + 1);
  else d += (size_t)xc * (Nz + 1);
  return d * sizeof(double);
}
static int cf_chunk(int Nx, int Nz, bool inverse) {
  int xc = std::min(Nx, 16);
  while (xc > 1 && cf_plane_lds(Nx, Nz, xc, inverse) > FNO_LDS_MAX) xc >>= 1;
  return xc;
}
// LDS of the solve kernel: per row 32 complex right-hand sides, 32 factor pairs and the sub-diagonal entry
static size_t cf_solve_lds(int n) { return (size_t)n * (4 * kCfTile + 1) * sizeof(double); }
static int cf_grid_check(const FnoChanflowGrid* g, int B) {
  if (!g) return fail(FNO_EINVAL, "chanflow step: null grid");
  if (B < 1 || B > 65535) return fail(FNO_EINVAL, "chanflow step: batch must be in 1..65535 (got %d)", B);
  if (g->Nx < 2 || g->Nx > 128 || g->Nz < 2 || g->Nz > 128)
    return fail(FNO_EUNSUPPORTED, "chanflow step: Nx and Nz must be in 2..128, the range of the in-LDS transforms (got Nx=%d, Nz=%d)",
                g->Nx, g->Nz);
  if (g->Ny < 3 || cf_solve_lds(g->Ny - 1) > FNO_LDS_MAX)
    return fail(FNO_EUNSUPPORTED, "chanflow step: Ny must be in 3..%d, a solve tile of all rows and its factors have to fit LDS (got %d)",
                (int)(FNO_LDS_MAX / cf_solve_lds(1)) + 1, g->Ny);
  if (!(g->dx > 0) || !(g->dz > 0)) return fail(FNO_EINVAL, "chanflow step: dx and dz must be positive");
  if (cf_plane_lds(g->Nx, g->Nz, 1, true) > FNO_LDS_MAX) return fail(FNO_EUNSUPPORTED, "chanflow step: plane does not fit LDS");
  return FNO_OK;
}
extern "C" size_t fno_chanflow_poisson_table_bytes(const FnoChanflowGrid* grid) {
  if (cf_grid_check(grid, 1) != FNO_OK) return 0;
  return cf_tab_layout(grid->Nx, grid->Ny, grid->Nz).total;
}
extern "C" int fno_chanflow_poisson_pack(const FnoChanflowGrid* grid, const double* y, const double* ym, const double* yg,
                                         double* packed, size_t packed_bytes) {
  LAUNCHCHK(cf_grid_check(grid, 1));
  if (!y || !ym || !yg || !packed) return fail(FNO_EINVAL, "fno_chanflow_poisson_pack: null array");
  const int Nx = grid->Nx, Ny = grid->Ny, Nz = grid->Nz, Nzh = Nz / 2 + 1, n = Ny - 1;
  const CfTabLayout l = cf_tab_layout(Nx, Ny, Nz);
  if (packed_bytes < l.total) return fail(FNO_ENOMEM, "fno_chanflow_poisson_pack: table needs %zu bytes, have %zu", l.total, packed_bytes);
  const double pi = 3.14159265358979323846;
  for (int m = 0; m < Nx; ++m) { packed[l.twx + 2 * m] = cos(2 * pi * m / Nx); packed[l.twx + 2 * m + 1] = -sin(2 * pi * m / Nx); }
  for (int m = 0; m < Nz; ++m) { packed[l.twz + 2 * m] = cos(2 * pi * m / Nz); packed[l.twz + 2 * m + 1] = -sin(2 * pi * m / Nz); }
  for (int k = 0; k < Nzh + 1 && l.wgt + k < l.trap; ++k) packed[l.wgt + k] = 0.0;
  for (int k = 0; k < Nzh; ++k) packed[l.wgt + k] = (k == 0 || 2 * k == Nz) ? 1.0 : 2.0;
  // trapezoid over [0, ym, 2] of the xz-mean profile, / 2 (control_env.py:249-259), as weights on the xz-SUMS of U rows 1..Ny-1
  for (int j = 0; j < l.sub - l.trap; ++j) packed[l.trap + j] = 0.0;
  for (int j = 0; j < n; ++j) {
    const double lo = j ? ym[j - 1] : 0.0, hi = (j + 1 < n) ? ym[j + 1] : 2.0;
    packed[l.trap + j] = 0.5 * (hi - lo) / 2.0 / ((double)Nx * Nz);
  }
  // DD (control_env.py:66-77): row j couples rows j-1 (sub) and j+1 (sup)
  std::vector<double> dg(n), sup(n);
  for (int j = 0; j < l.fac - l.sub; ++j) packed[l.sub + j] = 0.0;
  for (int j = 0; j < n; ++j) {
    const double hy = y[j + 1] - y[j], gu = yg[j + 2] - yg[j + 1], gl = yg[j + 1] - yg[j];
    dg[j] = -1.0 / hy * (1.0 / gu + 1.0 / gl);
    sup[j] = (j + 1 < n) ? 1.0 / hy / gu : 0.0;
    packed[l.sub + j] = j ? 1.0 / hy / gl : 0.0;
  }
  dg[0] += 1.0 / (y[1] - y[0]) / (yg[1] - yg[0]);
  dg[n - 1] += 1.0 / (y[Ny - 1] - y[Ny - 2]) / (yg[Ny] - yg[Ny - 1]);
  auto kmod = [pi](int k, int N, double d) {      // modified wavenumbers (:53-64)
    const int s = (k <= N / 2) ? k : k - N;
    return 2.0 * (cos(2 * pi * s / N) - 1.0) / (d * d);
  };
  double* fac = packed + l.fac;
  for (int c = 0; c < l.ntile * kCfTile; ++c) {
    const int tile = c / kCfTile, cl = c % kCfTile;
    const bool live = c < Nx * Nzh;
    const double kk = live ? kmod(c / Nzh, Nx, grid->dx) + kmod(c % Nzh, Nz, grid->dz) : 0.0;
    double cp = 0.0;
    for (int j = 0; j < n; ++j) {
      double* f = fac + (((size_t)tile * n + j) * kCfTile + cl) * 2;
      if (!live) { f[0] = 1.0; f[1] = 0.0; continue; }
      double d = dg[j] + kk;
      if (c == 0 && j == 0) d *= 1.5;                       // regularisation of the singular (0,0) system (:223-224)
      const double piv = d - packed[l.sub + j] * cp;
      f[0] = 1.0 / piv;
      cp = sup[j] / piv;
      f[1] = cp;
      if (!std::isfinite(f[0]) || !std::isfinite(f[1])) return fail(FNO_EINVAL, "fno_chanflow_poisson_pack: singular system (column %d, row %d)", c, j);
    }
  }
  return FNO_OK;
}

struct CfWs { double *F1[3], *Fs[3], *Xs[3]; double2* H; double* rowsum; size_t total; bool ok; };
static CfWs carve_cf(const FnoChanflowGrid* g, int B, void* ws, size_t ws_bytes) {
  CfWs w;
  const size_t su = (size_t)B * g->Nx * (g->Ny + 1) * g->Nz, sv = (size_t)B * g->Nx * g->Ny * g->Nz;
  auto up = [](size_t n) { return (n + 31) & ~(size_t)31; };
  double* p = (double*)ws;
  for (double** f : {w.F1, w.Fs, w.Xs}) {
    f[0] = p; p += up(su);
    f[1] = p; p += up(sv);
    f[2] = p; p += up(su);
  }
  w.H = (double2*)p; p += up((size_t)B * (g->Ny - 1) * g->Nx * (g->Nz / 2 + 1) * 2);
  w.rowsum = p; p += up((size_t)B * (g->Ny - 1));
  w.total = (size_t)((char*)p - (char*)ws);
  w.ok = ws_bytes >= w.total;
  return w;
}
extern "C" size_t fno_chanflow_step_workspace_bytes(const FnoChanflowGrid* grid, int B) {
  if (cf_grid_check(grid, B) != FNO_OK) return 0;
  return carve_cf(grid, B, nullptr, 0).total;
}
// everything the step entry points share: grid, dtype, table size, alignment, workspace
struct CfCall { ChanflowGeo geo; ChanflowTab tab; CfWs w; hipStream_t st; int ncol; };
static int cf_prepare(const char* who, const FnoChanflowGrid* g, int B, int dtype, const double* metrics, const double* table,
                      size_t table_bytes, std::initializer_list<const void*> need, std::initializer_list<const void*> opt, void* ws,
                      size_t ws_bytes, bool use_ws, void* stream, CfCall* c) {
  LAUNCHCHK(cf_grid_check(g, B));
  if (dtype != 1) return fail(FNO_EINVAL, "%s: the stepper's state is float64 only (dtype must be 1, got %d)", who, dtype);
  LAUNCHCHK(chanflow_geo(g, B, metrics, &c->geo));
  const CfTabLayout l = cf_tab_layout(g->Nx, g->Ny, g->Nz);
  if (!table || table_bytes != l.total)
    return fail(FNO_EINVAL, "%s: Poisson table of %zu bytes does not belong to this grid (%d x %d x %d needs %zu)", who, table_bytes,
                g->Nx, g->Ny, g->Nz, l.total);
  if (((uintptr_t)table & 15) || ((uintptr_t)metrics & 7)) return fail(FNO_EINVAL, "%s: table must be 16-byte aligned", who);
  for (const void* p : need)
    if (!p || ((uintptr_t)p & 7)) return fail(FNO_EINVAL, "%s: null or misaligned (8 B) tensor", who);
  for (const void* p : opt)
    if ((uintptr_t)p & 7) return fail(FNO_EINVAL, "%s: misaligned (8 B) tensor", who);
  c->tab = ChanflowTab{table, l.twx, l.twz, l.wgt, l.trap, l.sub, l.fac};
  c->ncol = g->Nx * (g->Nz / 2 + 1);
  c->st = (hipStream_t)stream;
  if (use_ws) {
    if (!ws || ((uintptr_t)ws & 15)) return fail(FNO_EINVAL, "%s: null or misaligned (16 B) workspace", who);
    c->w = carve_cf(g, B, ws, ws_bytes);
    if (!c->w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", c->w.total, ws_bytes);
  }
  return FNO_OK;
}
static ChanflowCFields cf_const(double* const* f) { return ChanflowCFields{f[0], f[1], f[2]}; }
static ChanflowFields cf_mut(double* const* f) { return ChanflowFields{f[0], f[1], f[2]}; }
// divergence of (X0 + ca F1 + cb Fs) -> h -> p_hat; writes the stage state to `out` when given
static int cf_poisson(const CfCall& c, ChanflowCFields X0, ChanflowCFields F1, ChanflowCFields Fs, double ca, double cb,
                      ChanflowFields out, const double* opV1, const double* opV2) {
  const ChanflowGeo& g = c.geo;
  ChanflowStageArgs a;
  a.X0 = X0; a.F1 = F1; a.Fs = Fs; a.out = out; a.opV1 = opV1; a.opV2 = opV2; a.ca = ca; a.cb = cb; a.h = c.w.H;
  a.xc = cf_chunk(g.Nx, g.Nz, false);
  LAUNCHCHK(launch("k_chanflow_stage", k_chanflow_stage, dim3(g.Ny - 1, g.B), dim3(256), cf_plane_lds(g.Nx, g.Nz, a.xc, false), c.st,
                   g, c.tab, a));
  return launch("k_chanflow_solve", k_chanflow_solve, dim3((c.ncol + kCfTile - 1) / kCfTile, g.B), dim3(256),
                cf_solve_lds(g.Ny - 1), c.st, g.Ny - 1, c.ncol, c.tab, c.w.H);
}
static int cf_correct(const CfCall& c, ChanflowCFields in, ChanflowFields out, double* rowsum) {
  const ChanflowGeo& g = c.geo;
  ChanflowCorrectArgs a;
  a.in = in; a.out = out; a.ph = c.w.H; a.rowsum = rowsum; a.xc = cf_chunk(g.Nx, g.Nz, true);
  return launch("k_chanflow_correct", k_chanflow_correct, dim3(g.Ny - 1, g.B), dim3(256), cf_plane_lds(g.Nx, g.Nz, a.xc, true), c.st,
                g, c.tab, a);
}
extern "C" int fno_chanflow_project(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const double* table,
                                    size_t table_bytes, void* U, void* V, void* W, void* ws, size_t ws_bytes, void* stream) {
  CfCall c;
  LAUNCHCHK(cf_prepare("fno_chanflow_project", grid, B, dtype, metrics, table, table_bytes, {U, V, W}, {}, ws, ws_bytes, true, stream, &c));
  const ChanflowCFields X{(const double*)U, (const double*)V, (const double*)W}, none{nullptr, nullptr, nullptr};
  LAUNCHCHK(cf_poisson(c, X, none, none, 0.0, 0.0, ChanflowFields{nullptr, nullptr, nullptr}, nullptr, nullptr));
  return cf_correct(c, X, ChanflowFields{(double*)U, (double*)V, (double*)W}, nullptr);
}
extern "C" int fno_chanflow_wall_pressure(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const double* table,
                                          size_t table_bytes, const void* U, const void* V, const void* W, const void* dpdx,
                                          void* p1, void* p2, void* P, void* ws, size_t ws_bytes, void* stream) {
  CfCall c;
  LAUNCHCHK(cf_prepare("fno_chanflow_wall_pressure", grid, B, dtype, metrics, table, table_bytes, {U, V, W, dpdx, p1, p2}, {P}, ws,
                       ws_bytes, true, stream, &c));
  const ChanflowCFields none{nullptr, nullptr, nullptr};
  LAUNCHCHK(chanflow_rhs_t<double>(c.geo, U, V, W, dpdx, 0.0, c.w.Fs[0], c.w.Fs[1], c.w.Fs[2], c.st));
  LAUNCHCHK(cf_poisson(c, cf_const(c.w.Fs), none, none, 0.0, 0.0, ChanflowFields{nullptr, nullptr, nullptr}, nullptr, nullptr));
  const int xc = cf_chunk(grid->Nx, grid->Nz, true);
  return launch("k_chanflow_pressure", k_chanflow_pressure, dim3(2 + (P ? grid->Ny - 1 : 0), B), dim3(256),
                cf_plane_lds(grid->Nx, grid->Nz, xc, true), c.st, c.geo, c.tab, (const double2*)c.w.H, (double*)p1, (double*)p2,
                (double*)P, xc);
}
extern "C" int fno_chanflow_rk3_step(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const double* table,
                                     size_t table_bytes, void* U, void* V, void* W, const void* opV1, const void* opV2, void* dpdx,
                                     const void* meanU0, double dt, void* ws, size_t ws_bytes, void* stream) {
  CfCall c;
  LAUNCHCHK(cf_prepare("fno_chanflow_rk3_step", grid, B, dtype, metrics, table, table_bytes, {U, V, W, opV1, opV2, dpdx, meanU0}, {},
                       ws, ws_bytes, true, stream, &c));
  if (!(dt > 0) || !std::isfinite(dt)) return fail(FNO_EINVAL, "fno_chanflow_rk3_step: dt must be positive and finite");
  const ChanflowCFields X{(const double*)U, (const double*)V, (const double*)W}, none{nullptr, nullptr, nullptr};
  const ChanflowFields Xo{(double*)U, (double*)V, (double*)W};
  const double *v1 = (const double*)opV1, *v2 = (const double*)opV2;
  const CfWs& w = c.w;
  // stage 1: X0 + dt 8/15 F(X0)
  LAUNCHCHK(chanflow_rhs_t<double>(c.geo, U, V, W, dpdx, 0.0, w.F1[0], w.F1[1], w.F1[2], c.st));
  LAUNCHCHK(cf_poisson(c, X, cf_const(w.F1), none, dt * 8 / 15, 0.0, cf_mut(w.Xs), v1, v2));
  LAUNCHCHK(cf_correct(c, cf_const(w.Xs), cf_mut(w.Xs), nullptr));
  // stage 2: X0 + dt (1/4 F1 + 5/12 F(X1))
  LAUNCHCHK(chanflow_rhs_t<double>(c.geo, w.Xs[0], w.Xs[1], w.Xs[2], dpdx, 0.0, w.Fs[0], w.Fs[1], w.Fs[2], c.st));
  LAUNCHCHK(cf_poisson(c, X, cf_const(w.F1), cf_const(w.Fs), dt * (1.0 / 4), dt * (5.0 / 12), cf_mut(w.Xs), v1, v2));
  LAUNCHCHK(cf_correct(c, cf_const(w.Xs), cf_mut(w.Xs), nullptr));
  // stage 3: X0 + dt (1/4 F1 + 3/4 F(X2)), corrected straight into the caller's state
  LAUNCHCHK(chanflow_rhs_t<double>(c.geo, w.Xs[0], w.Xs[1], w.Xs[2], dpdx, 0.0, w.Fs[0], w.Fs[1], w.Fs[2], c.st));
  LAUNCHCHK(cf_poisson(c, X, cf_const(w.F1), cf_const(w.Fs), dt * (1.0 / 4), dt * (3.0 / 4), cf_mut(w.Xs), v1, v2));
  LAUNCHCHK(cf_correct(c, cf_const(w.Xs), Xo, w.rowsum));
  return launch("k_chanflow_bulk", k_chanflow_bulk, dim3(grid->Nx, B), dim3(256), 0, c.st, c.geo, c.tab, (const double*)w.rowsum,
                (const double*)meanU0, dt, (double*)U, (double*)dpdx);
}
extern "C" int fno_chanflow_diagnostics(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const double* table,
                                        size_t table_bytes, const void* U, const void* V, const void* W, const void* p2, void* out,
                                        void* stream) {
  CfCall c;
  LAUNCHCHK(cf_prepare("fno_chanflow_diagnostics", grid, B, dtype, metrics, table, table_bytes, {U, V, W, out}, {p2}, nullptr, 0, false,
                       stream, &c));
  return launch("k_chanflow_diag", k_chanflow_diag, dim3(B), dim3(256), 0, c.st, c.geo, c.tab,
                ChanflowCFields{(const double*)U, (const double*)V, (const double*)W}, (const double*)p2, (double*)out);
}

// ===========================================================================
// Closed-loop control (run_control.py): observation / action bridges, two-level diagnostics, running statistics
// ===========================================================================
static int ctrl_plane_check(const char* who, int B, size_t plane, size_t stride) {
  if (B < 1 || B > 65535) return fail(FNO_EINVAL, "%s: batch must be in 1..65535 (got %d)", who, B);
  if (plane < 1 || plane > 0x3fffffffull) return fail(FNO_EINVAL, "%s: plane of %zu points", who, plane);
  if (stride < plane) return fail(FNO_EINVAL, "%s: batch stride %zu is shorter than the plane (%zu)", who, stride, plane);
  return FNO_OK;
}
extern "C" int fno_ctrl_encode(int B, size_t plane, const double* p, const double* mean, const double* std_, double eps, float* x,
                               size_t x_batch_stride, void* stream) {
  LAUNCHCHK(ctrl_plane_check("fno_ctrl_encode", B, plane, x_batch_stride));
  if (!p || !mean || !std_ || !x) return fail(FNO_EINVAL, "fno_ctrl_encode: null argument");
  if (((uintptr_t)p | (uintptr_t)mean | (uintptr_t)std_) & 7 || ((uintptr_t)x & 3)) return fail(FNO_EINVAL, "fno_ctrl_encode: misaligned tensor");
  return launch("k_ctrl_encode", k_ctrl_encode, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, plane, p, mean,
                std_, eps, x, x_batch_stride);
}
extern "C" int fno_ctrl_decode(int B, size_t plane, const float* y, size_t y_batch_stride, const double* mean, const double* std_,
                               double eps, double scale, double clip, int zero_mean, double* opV1, double* opV2, void* stream) {
  LAUNCHCHK(ctrl_plane_check("fno_ctrl_decode", B, plane, y_batch_stride));
  if (!y || !mean || !std_ || !opV2) return fail(FNO_EINVAL, "fno_ctrl_decode: null argument");
  if (((uintptr_t)opV1 | (uintptr_t)opV2 | (uintptr_t)mean | (uintptr_t)std_) & 7 || ((uintptr_t)y & 3))
    return fail(FNO_EINVAL, "fno_ctrl_decode: misaligned tensor");
  if (!std::isfinite(scale) || !(clip >= 0)) return fail(FNO_EINVAL, "fno_ctrl_decode: scale must be finite and clip >= 0 (0 = off)");
  CtrlDecodeArgs a;
  a.y = y; a.y_stride = y_batch_stride; a.plane = plane; a.mean = mean; a.sd = std_; a.eps = eps; a.scale = scale; a.clip = clip;
  a.use_scale = scale != 1.0; a.zero_mean = zero_mean ? 1 : 0; a.opV1 = opV1; a.opV2 = opV2;
  return launch("k_ctrl_decode", k_ctrl_decode, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
}
static size_t cf_diag2_bytes(const FnoChanflowGrid* g, int B) { return (size_t)B * (g->Ny + 1) * kCtrlDiagPart * sizeof(double); }
extern "C" size_t fno_chanflow_diagnostics2_workspace_bytes(const FnoChanflowGrid* grid, int B) {
  if (cf_grid_check(grid, B) != FNO_OK) return 0;
  return cf_diag2_bytes(grid, B);
}
extern "C" int fno_chanflow_diagnostics2(const FnoChanflowGrid* grid, int B, int dtype, const double* metrics, const double* table,
                                         size_t table_bytes, const void* U, const void* V, const void* W, const void* p2,
                                         const void* dpdx, void* out, size_t out_stride, void* ws, size_t ws_bytes, void* stream) {
  CfCall c;
  LAUNCHCHK(cf_prepare("fno_chanflow_diagnostics2", grid, B, dtype, metrics, table, table_bytes, {U, V, W, dpdx, out, ws}, {p2}, nullptr, 0,
                       false, stream, &c));
  if (out_stride < (size_t)kCtrlDiagOut) return fail(FNO_EINVAL, "fno_chanflow_diagnostics2: out stride %zu is shorter than a row (%d)", out_stride, kCtrlDiagOut);
  if (ws_bytes != cf_diag2_bytes(grid, B))
    return fail(FNO_EINVAL, "fno_chanflow_diagnostics2: workspace of %zu bytes does not belong to this grid and batch (%d x %d x %d, batch %d needs %zu)",
                ws_bytes, grid->Nx, grid->Ny, grid->Nz, B, cf_diag2_bytes(grid, B));
  LAUNCHCHK(launch("k_chanflow_diag_part", k_chanflow_diag_part, dim3(grid->Ny + 1, B), dim3(256), 0, c.st, c.geo, c.tab,
                   ChanflowCFields{(const double*)U, (const double*)V, (const double*)W}, (const double*)p2, (double*)ws));
  return launch("k_chanflow_diag_finish", k_chanflow_diag_finish, dim3(B), dim3(256), 0, c.st, c.geo, (const double*)ws, (const double*)dpdx,
                (double*)out, out_stride);
}
// ===========================================================================
// NSControlEnv2D: the 2-D periodic channel, fp64, one workgroup per environment with the state in LDS (k_ns2d.h)
// ===========================================================================
static size_t ns2d_lds_bytes(int n) { return ((size_t)7 * n + kNs2dRed) * sizeof(double); }
static int ns2d_prepare(const char* who, const FnoNs2dGrid* g, int B, std::initializer_list<const void*> need,
                        std::initializer_list<const void*> opt, Ns2dGeo* geo) {
  if (!g) return fail(FNO_EINVAL, "%s: null grid", who);
  if (B < 1) return fail(FNO_EINVAL, "%s: batch must be positive (got %d)", who, B);
  if (g->nx < 3 || g->ny < 3) return fail(FNO_EUNSUPPORTED, "%s: nx and ny must be at least 3 (got ny=%d, nx=%d)", who, g->ny, g->nx);
  if ((long long)g->nx * g->ny > kNs2dMaxPoints)
    return fail(FNO_EUNSUPPORTED, "%s: ny*nx = %lld exceeds %d points, the seven float64 planes of one environment have to fit LDS (160 KB per CU)",
                who, (long long)g->nx * g->ny, kNs2dMaxPoints);
  if (g->nit < 0) return fail(FNO_EINVAL, "%s: nit must not be negative (got %d)", who, g->nit);
  if (!(g->dx > 0) || !(g->dy > 0) || !(g->dt > 0) || !(g->rho > 0) || !std::isfinite(g->dx) || !std::isfinite(g->dy) ||
      !std::isfinite(g->dt) || !std::isfinite(g->rho))
    return fail(FNO_EINVAL, "%s: dx, dy, dt and rho must be positive and finite", who);
  for (const void* p : need)
    if (!p || ((uintptr_t)p & 7)) return fail(FNO_EINVAL, "%s: null or misaligned (8 B) tensor", who);
  for (const void* p : opt)
    if ((uintptr_t)p & 7) return fail(FNO_EINVAL, "%s: misaligned (8 B) tensor", who);
  *geo = Ns2dGeo{g->nx, g->ny, g->nit, g->dx, g->dy, g->dt, g->rho};
  return FNO_OK;
}
static int ns2d_loop_check(const char* who, double thre, int step_cap) {
  if (step_cap < 1 || step_cap > (1 << 30)) return fail(FNO_EINVAL, "%s: step_cap must be in 1..2^30 (got %d)", who, step_cap);
  if (std::isnan(thre)) return fail(FNO_EINVAL, "%s: u_diff_thre is NaN", who);
  return FNO_OK;
}
extern "C" int fno_ns2d_solve(const FnoNs2dGrid* grid, int B, void* p, void* u, void* v, void* un, void* vn, const void* F,
                              const void* nu, const void* bc_lo, const void* bc_hi, int max_step, double u_diff_thre, int step_cap,
                              int update_state, void* out, void* stream) {
  static_assert(FNO_NS2D_SOLVE_OUT == kNs2dSolveOut && FNO_NS2D_FIXED_OUT == kNs2dFixedOut && FNO_NS2D_DIAG_OUT == kNs2dDiagOut &&
                FNO_NS2D_MAX_POINTS == kNs2dMaxPoints, "ns2d constants of the header");
  Ns2dGeo geo;
  LAUNCHCHK(ns2d_prepare("fno_ns2d_solve", grid, B, {p, u, v, F, nu, out}, {un, vn, bc_lo, bc_hi}, &geo));
  LAUNCHCHK(ns2d_loop_check("fno_ns2d_solve", u_diff_thre, step_cap));
  Ns2dSolveArgs a;
  a.p = (double*)p; a.u = (double*)u; a.v = (double*)v; a.un = (double*)un; a.vn = (double*)vn;
  a.F = (const double*)F; a.nu = (const double*)nu; a.bc_lo = (const double*)bc_lo; a.bc_hi = (const double*)bc_hi;
  a.out = (double*)out; a.max_step = max_step; a.step_cap = step_cap; a.update = update_state ? 1 : 0; a.thre = u_diff_thre;
  return LV("k_ns2d_solve", 1, B), launch("k_ns2d_solve", k_ns2d_solve, dim3(B), dim3(kNs2dThreads), ns2d_lds_bytes(geo.nx * geo.ny),
                                          (hipStream_t)stream, geo, a);
}
extern "C" int fno_ns2d_fixed_mass(const FnoNs2dGrid* grid, int B, const void* p, const void* u, const void* v, const void* F,
                                   const void* nu, const void* target, const void* min_f, const void* max_f, const void* bc_lo,
                                   const void* bc_hi, double u_diff_thre, int step_cap, int max_bisect, double error_threshold,
                                   void* out, void* stream) {
  Ns2dGeo geo;
  LAUNCHCHK(ns2d_prepare("fno_ns2d_fixed_mass", grid, B, {p, u, v, F, nu, target, min_f, max_f, out}, {bc_lo, bc_hi}, &geo));
  LAUNCHCHK(ns2d_loop_check("fno_ns2d_fixed_mass", u_diff_thre, step_cap));
  if (max_bisect < 1 || max_bisect > 4096) return fail(FNO_EINVAL, "fno_ns2d_fixed_mass: max_bisect must be in 1..4096 (got %d)", max_bisect);
  if (std::isnan(error_threshold)) return fail(FNO_EINVAL, "fno_ns2d_fixed_mass: error_threshold is NaN");
  Ns2dFixedArgs a;
  a.p = (const double*)p; a.u = (const double*)u; a.v = (const double*)v; a.F = (const double*)F; a.nu = (const double*)nu;
  a.target = (const double*)target; a.min_f = (const double*)min_f; a.max_f = (const double*)max_f;
  a.bc_lo = (const double*)bc_lo; a.bc_hi = (const double*)bc_hi; a.out = (double*)out;
  a.step_cap = step_cap; a.max_bisect = max_bisect; a.thre = u_diff_thre; a.err_thre = error_threshold;
  return LV("k_ns2d_fixed_mass", 1, B), launch("k_ns2d_fixed_mass", k_ns2d_fixed_mass, dim3(B), dim3(kNs2dThreads),
                                               ns2d_lds_bytes(geo.nx * geo.ny), (hipStream_t)stream, geo, a);
}
extern "C" int fno_ns2d_diagnostics(const FnoNs2dGrid* grid, int B, const void* p, const void* u, const void* v, const void* nu,
                                    const void* dpdx, void* out, void* ptop, void* stream) {
  Ns2dGeo geo;
  LAUNCHCHK(ns2d_prepare("fno_ns2d_diagnostics", grid, B, {p, u, v, nu, out, ptop}, {dpdx}, &geo));
  if (geo.nx < 11 || geo.ny < 11)
    return fail(FNO_EUNSUPPORTED, "fno_ns2d_diagnostics: the divergence probe reads the fixed indices 10 and 9, so ny and nx must be at least 11 (got ny=%d, nx=%d)",
                geo.ny, geo.nx);
  return LV("k_ns2d_diag", 1, B), launch("k_ns2d_diag", k_ns2d_diag, dim3(B), dim3(256), 0, (hipStream_t)stream, geo, (const double*)p,
                                         (const double*)u, (const double*)v, (const double*)nu, (const double*)dpdx, (double*)out,
                                         (double*)ptop);
}
extern "C" int fno_ctrl_stats_update(const FnoCtrlStats* tab, int nfields, long long count, void* stream) {
  static_assert(FNO_CTRL_STATS_MAX == kCtrlStatsMax, "statistics table size");
  if (!tab) return fail(FNO_EINVAL, "fno_ctrl_stats_update: null table");
  if (nfields < 1 || nfields > kCtrlStatsMax)
    return fail(FNO_EINVAL, "fno_ctrl_stats_update: 1..%d fields per launch (got %d)", kCtrlStatsMax, nfields);
  if (count < 1) return fail(FNO_EINVAL, "fno_ctrl_stats_update: count is the number of snapshots including this one (got %lld)", count);
  CtrlStatsTab t;
  size_t most = 0;
  for (int f = 0; f < kCtrlStatsMax; ++f) {
    const bool on = f < nfields;
    t.x[f] = on ? tab->x[f] : nullptr; t.mean[f] = on ? tab->mean[f] : nullptr; t.m2[f] = on ? tab->m2[f] : nullptr; t.n[f] = on ? tab->n[f] : 0;
    if (!on) continue;
    if (!t.x[f] || !t.mean[f] || !t.m2[f] || (((uintptr_t)t.x[f] | (uintptr_t)t.mean[f] | (uintptr_t)t.m2[f]) & 7) || t.n[f] < 1)
      return fail(FNO_EINVAL, "fno_ctrl_stats_update: field %d is null, misaligned or empty", f);
    most = std::max(most, t.n[f]);
  }
  const unsigned gx = (unsigned)std::min<size_t>((most + 255) / 256, 4096);
  return launch("k_ctrl_stats", k_ctrl_stats, dim3(gx, nfields), dim3(256), 0, (hipStream_t)stream, t, (double)count);
}

// ===========================================================================
// optimal-observer policy (run_control.py:186-224): the objective and the Adam step on the wall action (k_action_opt.h)
// ===========================================================================
static int act_check(const char* who, int B, size_t plane, size_t stride, const double* mean, const double* std_, double eps) {
  LAUNCHCHK(ctrl_plane_check(who, B, plane, stride));
  if (!mean || !std_) return fail(FNO_EINVAL, "%s: null statistics", who);
  if (((uintptr_t)mean | (uintptr_t)std_) & 7) return fail(FNO_EINVAL, "%s: misaligned statistics", who);
  if (!std::isfinite(eps)) return fail(FNO_EINVAL, "%s: eps must be finite", who);
  return FNO_OK;
}
static int act_obj_chunks(int B, int P, size_t plane, size_t* nchunk) {
  LAUNCHCHK(ctrl_plane_check("fno_ctrl_action_objective", B, plane, plane));
  if (P < 1 || P > 64) return fail(FNO_EINVAL, "fno_ctrl_action_objective: 1..64 predicted planes (got %d)", P);
  if ((size_t)P * plane > 0x3fffffffull) return fail(FNO_EINVAL, "fno_ctrl_action_objective: %d planes of %zu points", P, plane);
  *nchunk = ((size_t)P * plane + kActChunk - 1) / kActChunk;
  return FNO_OK;
}
extern "C" size_t fno_ctrl_action_workspace_bytes(int B, int P, size_t plane) {
  size_t nchunk;
  if (act_obj_chunks(B, P, plane, &nchunk) != FNO_OK) return 0;
  return (size_t)B * nchunk * 2 * sizeof(double);
}
extern "C" int fno_ctrl_action_begin(int B, size_t plane, const double* opV2_0, const double* mean, const double* std_, double eps,
                                     float* a, float* x, size_t x_batch_stride, void* stream) {
  LAUNCHCHK(act_check("fno_ctrl_action_begin", B, plane, x_batch_stride, mean, std_, eps));
  if (!opV2_0 || !a || !x) return fail(FNO_EINVAL, "fno_ctrl_action_begin: null argument");
  if (((uintptr_t)opV2_0 & 7) || (((uintptr_t)a | (uintptr_t)x) & 3)) return fail(FNO_EINVAL, "fno_ctrl_action_begin: misaligned tensor");
  return launch("k_act_begin", k_act_begin, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, plane, opV2_0,
                ActStats{mean, std_, eps}, a, x, x_batch_stride);
}
extern "C" int fno_ctrl_action_objective(int B, int P, size_t plane, const float* y, const float* a, const double* mean,
                                         const double* std_, double eps, double reg, double* parts, float* dy, void* ws,
                                         size_t ws_bytes, void* stream) {
  size_t nchunk;
  LAUNCHCHK(act_obj_chunks(B, P, plane, &nchunk));
  LAUNCHCHK(act_check("fno_ctrl_action_objective", B, plane, plane, mean, std_, eps));
  if (!y || !a || !parts || !dy || !ws) return fail(FNO_EINVAL, "fno_ctrl_action_objective: null argument");
  if ((((uintptr_t)y | (uintptr_t)a | (uintptr_t)dy) & 3) || (((uintptr_t)parts | (uintptr_t)ws) & 7))
    return fail(FNO_EINVAL, "fno_ctrl_action_objective: misaligned tensor");
  if (!std::isfinite(reg)) return fail(FNO_EINVAL, "fno_ctrl_action_objective: reg must be finite");
  if (ws_bytes != (size_t)B * nchunk * 2 * sizeof(double))
    return fail(FNO_EINVAL, "fno_ctrl_action_objective: workspace of %zu bytes does not belong to batch %d, %d planes of %zu (needs %zu)",
                ws_bytes, B, P, plane, (size_t)B * nchunk * 2 * sizeof(double));
  ActObjArgs o;
  o.y = y; o.a = a; o.s = ActStats{mean, std_, eps}; o.plane = plane; o.total = (size_t)P * plane; o.nchunk = (int)nchunk; o.reg = reg;
  o.ws = (double*)ws; o.parts = parts; o.dy = dy;
  LAUNCHCHK(launch("k_act_obj_part", k_act_obj_part, dim3((unsigned)nchunk, B), dim3(256), 0, (hipStream_t)stream, o));
  return launch("k_act_obj_dy", k_act_obj_dy, dim3((unsigned)nchunk, B), dim3(256), 0, (hipStream_t)stream, o);
}
extern "C" int fno_ctrl_action_update(int B, size_t plane, const float* dx, const double* parts, const double* mean,
                                      const double* std_, double eps, double reg, double lr, double beta1, double beta2,
                                      double adam_eps, int step, float* a, float* exp_avg, float* exp_avg_sq, float* x,
                                      size_t x_batch_stride, void* stream) {
  LAUNCHCHK(act_check("fno_ctrl_action_update", B, plane, x_batch_stride, mean, std_, eps));
  if (step < 1) return fail(FNO_EINVAL, "fno_ctrl_action_update: step must be >= 1 (got %d)", step);
  if (!dx || !parts || !a || !exp_avg || !exp_avg_sq || !x) return fail(FNO_EINVAL, "fno_ctrl_action_update: null argument");
  if ((((uintptr_t)dx | (uintptr_t)a | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)x) & 3) || ((uintptr_t)parts & 7))
    return fail(FNO_EINVAL, "fno_ctrl_action_update: misaligned tensor");
  if (!std::isfinite(reg) || !std::isfinite(lr) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(adam_eps >= 0))
    return fail(FNO_EINVAL, "fno_ctrl_action_update: need finite reg and lr, betas in [0, 1) and eps >= 0");
  const AdamHyper h = adam_hyper(lr, beta1, beta2, adam_eps, 0.0);
  float sc[2];
  fno_adam_scalars(lr, beta1, beta2, step, sc);
  ActUpdateArgs u;
  u.dx = dx; u.parts = parts; u.s = ActStats{mean, std_, eps}; u.plane = plane; u.x_stride = x_batch_stride; u.reg = reg;
  u.beta2 = h.beta2; u.eps = h.eps; u.step_size = sc[0]; u.bc2_sqrt = sc[1]; u.omb1 = h.omb1; u.omb2 = h.omb2;
  u.first = step == 1; u.a = a; u.m = exp_avg; u.v = exp_avg_sq; u.x = x;
  return launch("k_act_update", k_act_update, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, u);
}
extern "C" int fno_ctrl_action_finish(int B, size_t plane, const float* a, double* opV2, void* stream) {
  LAUNCHCHK(ctrl_plane_check("fno_ctrl_action_finish", B, plane, plane));
  if (!a || !opV2) return fail(FNO_EINVAL, "fno_ctrl_action_finish: null argument");
  if (((uintptr_t)a & 3) || ((uintptr_t)opV2 & 7)) return fail(FNO_EINVAL, "fno_ctrl_action_finish: misaligned tensor");
  return launch("k_act_finish", k_act_finish, dim3(B), dim3(256), 0, (hipStream_t)stream, plane, a, opV2);
}

// ===========================================================================
// optimal-policy-observer policy (run_control.py:162-185): the glue between the policy network and the observer (k_policy_opt.h)
// ===========================================================================
static int pol_check(const char* who, int B, size_t plane, std::initializer_list<const void*> f32, std::initializer_list<const void*> f64) {
  LAUNCHCHK(ctrl_plane_check(who, B, plane, plane));
  for (const void* p : f32) {
    if (!p) return fail(FNO_EINVAL, "%s: null argument", who);
    if ((uintptr_t)p & 3) return fail(FNO_EINVAL, "%s: misaligned tensor", who);
  }
  for (const void* p : f64) {
    if (!p) return fail(FNO_EINVAL, "%s: null argument", who);
    if ((uintptr_t)p & 7) return fail(FNO_EINVAL, "%s: misaligned tensor", who);
  }
  return FNO_OK;
}
extern "C" int fno_ctrl_policy_begin(int B, size_t plane, const double* opV2_0, const double* p2, float* a0, float* pin, void* stream) {
  LAUNCHCHK(pol_check("fno_ctrl_policy_begin", B, plane, {a0, pin}, {opV2_0, p2}));
  return launch("k_pol_begin", k_pol_begin, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, plane, opV2_0,
                p2, a0, pin);
}
extern "C" int fno_ctrl_policy_compose(int B, size_t plane, const float* a0, const float* res, float* x, double* opV2, void* stream) {
  LAUNCHCHK(pol_check("fno_ctrl_policy_compose", B, plane, {a0, res, x}, {opV2}));
  return launch("k_pol_compose", k_pol_compose, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, plane, a0,
                res, x, opV2);
}
extern "C" int fno_ctrl_policy_grad(int B, size_t plane, const float* dx, const float* x, const double* parts, double reg, float* g,
                                    void* stream) {
  LAUNCHCHK(pol_check("fno_ctrl_policy_grad", B, plane, {dx, x, g}, {parts}));
  if (!std::isfinite(reg)) return fail(FNO_EINVAL, "fno_ctrl_policy_grad: reg must be finite");
  return launch("k_pol_grad", k_pol_grad, dim3((unsigned)((plane + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, plane, dx, x,
                parts, reg, g);
}

// ===========================================================================
// RNO cell gates (neuralop/models/rno.py:254-260)
// ===========================================================================
static const int kGateGrid = 2048;
extern "C" int fno_rno_gate_partials(void) { return kGateGrid; }
static int gate_check(size_t n, std::initializer_list<const void*> ptrs) {
  if (n == 0 || n % 4 != 0) return fail(FNO_EINVAL, "rno gates: element count must be a positive multiple of 4 (got %zu)", n);
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & 15)) return fail(FNO_EINVAL, "rno gates: null or unaligned (16 B) tensor");
  return FNO_OK;
}
extern "C" int fno_rno_reset_gate_forward(size_t n, const float* a3, const float* a4, const float* b2, const float* h,
                                          float* r, float* rh, void* stream) {
  LAUNCHCHK(gate_check(n, {a3, a4, h, r, rh}));
  if (!b2) return fail(FNO_EINVAL, "rno gates: null bias");
  return launch("k_rno_reset_fwd", k_rno_reset_fwd, dim3(kGateGrid), dim3(256), 0, (hipStream_t)stream, (const float4*)a3,
                (const float4*)a4, b2, (const float4*)h, (float4*)r, (float4*)rh, n / 4);
}
extern "C" int fno_rno_reset_gate_backward(size_t n, const float* d_rh, const float* r, const float* h, float* d_s,
                                           float* d_h, double* db_partials, void* stream) {
  LAUNCHCHK(gate_check(n, {d_rh, r, h, d_s, d_h}));
  if (!db_partials) return fail(FNO_EINVAL, "rno gates: null partial buffer");
  return launch("k_rno_reset_bwd", k_rno_reset_bwd, dim3(kGateGrid), dim3(256), 0, (hipStream_t)stream, (const float4*)d_rh,
                (const float4*)r, (const float4*)h, (float4*)d_s, (float4*)d_h, db_partials, n / 4);
}
extern "C" int fno_rno_output_gate_forward(size_t n, const float* a1, const float* a2, const float* b1, const float* a7,
                                           const float* a8, const float* b4, const float* a5, const float* a6,
                                           const float* b3, const float* h, float* z, float* z2, float* s3, float* h_new,
                                           void* stream) {
  LAUNCHCHK(gate_check(n, {a1, a2, a7, a8, a5, a6, h, z, z2, s3, h_new}));
  if (!b1 || !b4 || !b3) return fail(FNO_EINVAL, "rno gates: null bias");
  RnoOutArgs a;
  a.a1 = (const float4*)a1; a.a2 = (const float4*)a2; a.a7 = (const float4*)a7; a.a8 = (const float4*)a8;
  a.a5 = (const float4*)a5; a.a6 = (const float4*)a6; a.h = (const float4*)h; a.b1 = b1; a.b4 = b4; a.b3 = b3;
  a.z = (float4*)z; a.z2 = (float4*)z2; a.s3 = (float4*)s3; a.hn = (float4*)h_new; a.n4 = n / 4;
  return launch("k_rno_out_fwd", k_rno_out_fwd, dim3(kGateGrid), dim3(256), 0, (hipStream_t)stream, a);
}
extern "C" int fno_rno_output_gate_backward(size_t n, const float* g, const float* z, const float* z2, const float* s3,
                                            const float* h, float* d_s1, float* d_s7, float* d_s3, float* d_h,
                                            double* db_partials, void* stream) {
  LAUNCHCHK(gate_check(n, {g, z, z2, s3, h, d_s1, d_s7, d_s3, d_h}));
  if (!db_partials) return fail(FNO_EINVAL, "rno gates: null partial buffer");
  RnoOutBwdArgs a;
  a.g = (const float4*)g; a.z = (const float4*)z; a.z2 = (const float4*)z2; a.s3 = (const float4*)s3; a.h = (const float4*)h;
  a.ds1 = (float4*)d_s1; a.ds7 = (float4*)d_s7; a.ds3 = (float4*)d_s3; a.dh = (float4*)d_h; a.db_part = db_partials;
  a.n4 = n / 4;
  return launch("k_rno_out_bwd", k_rno_out_bwd, dim3(kGateGrid), dim3(256), 0, (hipStream_t)stream, a);
}

// the dropout scale field the kernels regenerate (tests / oracles): out[e] = 0 or 1 / (1 - p)
__global__ void __launch_bounds__(256) k_drop_scale(float* __restrict__ out, size_t n, const unsigned* __restrict__ seed, float p) {
  const DropCfg dc = drop_cfg(seed, p);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) out[e] = drop_scale(dc, e);
}
extern "C" int fno_dropout_scale(size_t n, float drop_p, const unsigned* seed, float* out, void* stream) {
  if (!seed || !out || drop_p < 0.f || drop_p >= 1.f) return fail(FNO_EINVAL, "fno_dropout_scale: bad argument");
  if (n == 0) return FNO_OK;
  const int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)8 * dev_ncu());
  return launch("k_drop_scale", k_drop_scale, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, n, seed, drop_p);
}

// ===========================================================================
// Pointwise (1x1) channel mix with fused bias / residual add, forward and backward: the Conv1d(k=1) next to every
// spectral convolution of the observer models (libs/models/pino_models/pinobserver.py:183-184, 221-226:
// `sp_convs[i](x) + ws[i](x)`; neuralop/models/rno.py:222-228) for shapes the block stacks do not cover
// (odd last dimension).  Same tile kernels as the FNO block, without any spectral row pass.
// ===========================================================================
static int pw_check(int B, int C, size_t PW) {
  if (B < 1 || PW < 1) return fail(FNO_EINVAL, "pointwise: bad shape");
  if (C != 32 && C != 64) return fail(FNO_EUNSUPPORTED, "pointwise: 32 or 64 channels (got %d)", C);
  if (PW % 128 != 0) return fail(FNO_EUNSUPPORTED, "pointwise: plane of %zu elements does not tile by 128", PW);
  if (PW > (size_t)1 << 30 || (size_t)B * (PW / 128) > (size_t)1 << 30) return fail(FNO_EUNSUPPORTED, "pointwise: tensor too large");
  return FNO_OK;
}
// a FnoModelPlan shell carrying what the launch helpers read (tile size, CU count, width)
struct PwShell : FnoModelPlan {
  explicit PwShell(int C) {
    memset(&d, 0, sizeof(d));
    d.C = C;
    NPX = 128;
    loose = false;
    ncu = dev_ncu();
  }
};
extern "C" size_t fno_pointwise_workspace_bytes(int C) {
  const int grid = 2 * dev_ncu();
  return ((size_t)grid * 2 * C * C + (size_t)grid * C) * sizeof(float) + 1024;
}
extern "C" int fno_pointwise_forward(int B, int C, size_t PW, const float* x, const float* w, const float* bias,
                                     const float* addend, int input_gelu, float* y, void* stream) {
  LAUNCHCHK(pw_check(B, C, PW));
  if (!x || !w || !y) return fail(FNO_EINVAL, "fno_pointwise_forward: null argument");
  PwShell p(C);
  PwFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.bias = bias; a.add = addend; a.u = y; a.act_in = input_gelu ? 1 : 0;
  a.PW = (int)PW; a.W = 128; a.P = (int)(PW / 128);
  a.tiles_per_plane = (int)(PW / 128); a.ntiles = B * a.tiles_per_plane;
  return launch_block(&p, (hipStream_t)stream, blk_fwd_grid(&p, a.ntiles), a);
}
extern "C" int fno_pointwise_backward(int B, int C, size_t PW, const float* x, const float* w, const float* dy,
                                      const float* dx_addend, int input_gelu, float* dx, float* dw, float* dbias, void* ws,
                                      size_t ws_bytes, void* stream) {
  LAUNCHCHK(pw_check(B, C, PW));
  if (!x || !w || !dy || !dw || !ws) return fail(FNO_EINVAL, "fno_pointwise_backward: null argument");
  if (ws_bytes < fno_pointwise_workspace_bytes(C)) return fail(FNO_ENOMEM, "workspace too small");
  PwShell p(C);
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)(PW / 128), ntiles = B * tiles;
  const int grid = std::min(ntiles, FNO_GRID_BWD * p.ncu);
  const int ks = bbwd_ksplit(&p);
  Carver c(ws, ws_bytes);
  float* dw_part = c.take<float>((size_t)grid * ks * C * C);
  float* db_part = c.take<float>((size_t)grid * C);
  if (!c.ok) return fail(FNO_ENOMEM, "workspace too small");
  BlkBwdArgs a;
  memset(&a, 0, sizeof(a));
  if (dx_addend && !dx) return fail(FNO_EINVAL, "fno_pointwise_backward: dx_addend without dx");
  a.g = dy; a.uin = x; a.w = w; a.gout = dx; a.gadd = dx_addend; a.act_in = input_gelu ? 1 : 0;
  a.dw_part = dw_part; a.db_part = db_part;
  a.PW = (int)PW; a.W = 128; a.P = tiles; a.tiles_per_plane = tiles; a.ntiles = ntiles;
  LAUNCHCHK(launch_bbwd(&p, st, grid, a));
  JobList jobs;
  jobs.add(dw_part, dw, grid * ks, C, C, C, C);
  if (dbias) jobs.add(db_part, dbias, grid, 1, C, C, C);
  return jobs.run(st);
}

// ===========================================================================
// Projection head on its own:  y = W2 gelu(W1 x + b1) + b2  (x (B, C, PW), hidden 128 or 256, one output channel).
// The observer models end in exactly this MLP (libs/models/pino_models/pinobserver.py:231-233, 270-273:
// fc1 -> act -> fc2), applied there on channels-last tensors through nn.Linear; the kernels are the FNO
// projection kernels (hidden tensor kept in MFMA accumulators, backward recomputes it).
// ===========================================================================
struct ProjWs { unsigned short *wa1, *wa3; float *dw1_part, *db1_part, *dw2_part, *db2_part; size_t total; bool ok; };
static ProjWs carve_proj(int C, int HID, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  const int grid = FNO_GRID_BWD * dev_ncu();
  ProjWs w;
  w.wa1 = c.take<unsigned short>((size_t)(HID / 32) * (C / 16) * 3 * 64 * 8);
  w.wa3 = c.take<unsigned short>((size_t)(HID / 32) * 2 * (C / 32) * 3 * 64 * 8);
  w.dw1_part = c.take<float>((size_t)grid * HID * C);
  w.db1_part = c.take<float>((size_t)grid * 4 * HID);
  w.dw2_part = c.take<float>((size_t)grid * 4 * PROJ_MAXCO * HID);
  w.db2_part = c.take<float>((size_t)64 * PROJ_MAXCO);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
static int proj_check(int B, int C, int HID, int CO, size_t PW) {
  LAUNCHCHK(pw_check(B, C, PW));
  if (HID != 128 && HID != 256) return fail(FNO_EUNSUPPORTED, "projection: hidden width 128 or 256 (got %d)", HID);
  if (CO < 1 || CO > PROJ_MAXCO) return fail(FNO_EUNSUPPORTED, "projection: 1..%d output channels (got %d)", PROJ_MAXCO, CO);
  return FNO_OK;
}
extern "C" size_t fno_projection_workspace_bytes(int C, int hidden) {
  if ((C != 32 && C != 64) || (hidden != 128 && hidden != 256)) return 0;
  return carve_proj(C, hidden, nullptr, 0).total;
}
// (2..PROJ_MAXCO output channels - PlanePredHead, pinobserver.py:257-273: fc2 -> out_dim * plane_num - run as NCO = PROJ_MAXCO rows)
template <int C, int HID, bool RELU, int NCO = 1>
static int proj_fwd_launch(hipStream_t st, int grid, const ProjFwdArgs& a) {
  if (!g_gemm_x3)
    return GT(1), launch("k_proj_fwd", k_proj_fwd<C, HID, 128, NCO, RELU>, dim3(grid), dim3(512), proj_fwd_lds_bytes(C, HID, NCO), st, a);
  return GT(3), launch("k_proj_fwd", k_proj_fwd_x3<C, HID, 128, NCO, RELU>, dim3(grid), dim3(512), proj_fwd_x3_lds_bytes(C, HID, NCO), st, a);
}
template <int C, int HID, bool RELU>
static int proj_bwd_launch(hipStream_t st, int grid, const ProjBwdArgs& a) {
  if (!g_gemm_x3)      // exact-fp32 mode: the first-generation kernel
    return GT(1), launch("k_proj_bwd", k_proj_bwd<C, HID, 128, 1, RELU>, dim3(grid), dim3(512), proj_bwd_lds_bytes(C, HID, 128, 1), st, a);
  return GT(3), launch("k_proj_bwd", k_proj_bwd_t<C, HID, RELU>, dim3(grid), dim3(512), proj_bwd_t_lds_bytes(C, a), st, a);
}
// several output channels: the backward runs on the exact-fp32 first-generation kernel in both modes (the split-precision ones
// are built for one)
template <int C, int HID>
static int proj_bwd_launch_mo(hipStream_t st, int grid, const ProjBwdArgs& a) {
  return GT(1), launch("k_proj_bwd", k_proj_bwd<C, HID, 128, PROJ_MAXCO>, dim3(grid), dim3(512), proj_bwd_lds_bytes(C, HID, 128, PROJ_MAXCO), st, a);
}
static int proj_act_check(int hidden, int act) {
  if (act != FNO_ACT_GELU && act != FNO_ACT_RELU) return fail(FNO_EINVAL, "projection: hidden_act %d (FNO_ACT_GELU or FNO_ACT_RELU)", act);
  if (act == FNO_ACT_RELU && hidden != 256) return fail(FNO_EUNSUPPORTED, "projection: the ReLU head is built for hidden width 256 (got %d)", hidden);
  return FNO_OK;
}
extern "C" int fno_projection_forward_act(int B, int C, int hidden, int Cout, size_t PW, const float* x, const float* w1,
                                          const float* b1, const float* w2, const float* b2, int hidden_act, float* y,
                                          void* stream) {
  LAUNCHCHK(proj_check(B, C, hidden, Cout, PW));
  LAUNCHCHK(proj_act_check(hidden, hidden_act));
  if (!x || !w1 || !b1 || !w2 || !b2 || !y) return fail(FNO_EINVAL, "fno_projection_forward: null argument");
  ProjFwdArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.x = x; pa.w1 = w1; pa.b1 = b1; pa.w2 = w2; pa.b2 = b2; pa.y = y; pa.PW = (int)PW; pa.CO = Cout;
  pa.tiles_per_plane = (int)(PW / 128); pa.ntiles = B * pa.tiles_per_plane;
  const int grid = std::min(pa.ntiles, FNO_GRID_PF * dev_ncu());
  hipStream_t st = (hipStream_t)stream;
  if (Cout > 1) {
    if (hidden_act != FNO_ACT_GELU) return fail(FNO_EUNSUPPORTED, "projection: several output channels with the GELU head only");
    if (C == 32) return hidden == 128 ? proj_fwd_launch<32, 128, false, PROJ_MAXCO>(st, grid, pa) : proj_fwd_launch<32, 256, false, PROJ_MAXCO>(st, grid, pa);
    return hidden == 128 ? proj_fwd_launch<64, 128, false, PROJ_MAXCO>(st, grid, pa) : proj_fwd_launch<64, 256, false, PROJ_MAXCO>(st, grid, pa);
  }
  if (hidden_act == FNO_ACT_RELU) return C == 32 ? proj_fwd_launch<32, 256, true>(st, grid, pa) : proj_fwd_launch<64, 256, true>(st, grid, pa);
  if (C == 32) return hidden == 128 ? proj_fwd_launch<32, 128, false>(st, grid, pa) : proj_fwd_launch<32, 256, false>(st, grid, pa);
  return hidden == 128 ? proj_fwd_launch<64, 128, false>(st, grid, pa) : proj_fwd_launch<64, 256, false>(st, grid, pa);
}
extern "C" int fno_projection_forward(int B, int C, int hidden, int Cout, size_t PW, const float* x, const float* w1,
                                      const float* b1, const float* w2, const float* b2, float* y, void* stream) {
  return fno_projection_forward_act(B, C, hidden, Cout, PW, x, w1, b1, w2, b2, FNO_ACT_GELU, y, stream);
}
extern "C" int fno_projection_backward_act(int B, int C, int hidden, int Cout, size_t PW, const float* x, const float* w1,
                                           const float* b1, const float* w2, const float* dy, int hidden_act, float* dx,
                                           float* dw1, float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes,
                                           void* stream) {
  LAUNCHCHK(proj_check(B, C, hidden, Cout, PW));
  LAUNCHCHK(proj_act_check(hidden, hidden_act));
  if (!x || !w1 || !b1 || !w2 || !dy || !dx || !dw1 || !db1 || !dw2 || !db2 || !ws)
    return fail(FNO_EINVAL, "fno_projection_backward: null argument");
  ProjWs w = carve_proj(C, hidden, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  const bool split = Cout == 1 && g_gemm_x3;      // k_proj_bwd_t reads W1 as split-precision fragments
  if (split) LAUNCHCHK(pack_w1_x3(st, w1, w.wa1, w.wa3, hidden, C));
  ProjBwdArgs pb;
  memset(&pb, 0, sizeof(pb));
  pb.x = x; pb.dy = dy; pb.w1 = w1; pb.b1 = b1; pb.w2 = w2; pb.gout = dx;
  if (split) { pb.wa1 = w.wa1; pb.wa3 = w.wa3; }
  pb.dw1_part = w.dw1_part; pb.db1_part = w.db1_part; pb.dw2_part = w.dw2_part;
  pb.PW = (int)PW; pb.W = 128; pb.P = (int)(PW / 128); pb.CO = Cout;
  pb.tiles_per_plane = (int)(PW / 128); pb.ntiles = B * pb.tiles_per_plane;
  const int grid = std::min(pb.ntiles, FNO_GRID_BWD * dev_ncu());
  if (Cout > 1) {
    if (hidden_act != FNO_ACT_GELU) return fail(FNO_EUNSUPPORTED, "projection: several output channels with the GELU head only");
    if (C == 32) LAUNCHCHK((hidden == 128 ? proj_bwd_launch_mo<32, 128>(st, grid, pb) : proj_bwd_launch_mo<32, 256>(st, grid, pb)));
    else LAUNCHCHK((hidden == 128 ? proj_bwd_launch_mo<64, 128>(st, grid, pb) : proj_bwd_launch_mo<64, 256>(st, grid, pb)));
  } else
  if (hidden_act == FNO_ACT_RELU) LAUNCHCHK((C == 32 ? proj_bwd_launch<32, 256, true>(st, grid, pb) : proj_bwd_launch<64, 256, true>(st, grid, pb)));
  else if (C == 32) LAUNCHCHK((hidden == 128 ? proj_bwd_launch<32, 128, false>(st, grid, pb) : proj_bwd_launch<32, 256, false>(st, grid, pb)));
  else LAUNCHCHK((hidden == 128 ? proj_bwd_launch<64, 128, false>(st, grid, pb) : proj_bwd_launch<64, 256, false>(st, grid, pb)));
  LAUNCHCHK(launch("k_channel_sums", k_channel_sums, dim3(64, Cout), dim3(256), 0, st, dy, w.db2_part, B, Cout, (int)PW));
  JobList jobs;
  jobs.add(w.dw1_part, dw1, grid, hidden, C, C, C);
  jobs.add(w.db1_part, db1, grid * 4, 1, hidden, hidden, hidden);
  jobs.add(w.dw2_part, dw2, grid * 4, Cout, hidden, hidden, hidden);
  jobs.add(w.db2_part, db2, 64, 1, Cout, Cout, Cout);
  return jobs.run(st);
}
extern "C" int fno_projection_backward(int B, int C, int hidden, int Cout, size_t PW, const float* x, const float* w1,
                                       const float* b1, const float* w2, const float* dy, float* dx, float* dw1,
                                       float* db1, float* dw2, float* db2, void* ws, size_t ws_bytes, void* stream) {
  return fno_projection_backward_act(B, C, hidden, Cout, PW, x, w1, b1, w2, dy, FNO_ACT_GELU, dx, dw1, db1, dw2, db2, ws,
                                     ws_bytes, stream);
}

// ===========================================================================
// Channel MLP of an FNO block built with use_mlp=True:  y = [gelu]( gelu(W2 gelu(W1 u + b1) + b2) + g (.) x )
// (neuralop/models/fno_block.py:123-170, mlp.py:26-54, skip_connections.py:38-74; k_channel_mlp.h).  Exact-fp32 MFMA in
// either GEMM mode.
// ===========================================================================
static int cmlp_check(int B, int C, int HID, size_t PW) {
  LAUNCHCHK(pw_check(B, C, PW));
  if (!((C == 64 && (HID == 32 || HID == 64)) || (C == 32 && HID == 32)))
    return fail(FNO_EUNSUPPORTED, "channel MLP: (channels, hidden) is one of (64, 32), (64, 64), (32, 32) (got (%d, %d))", C, HID);
  return FNO_OK;
}
struct CmlpWs { float *dw1_part, *db1_part, *dw2_part, *db2_part, *dg_part; int grid, ks; size_t total; bool ok; };
static CmlpWs carve_cmlp(int C, int HID, int B, size_t PW, void* ws, size_t ws_bytes) {
  Carver c(ws, ws_bytes);
  CmlpWs w;
  w.grid = (int)std::min<size_t>((size_t)B * (PW / 128), (size_t)FNO_GRID_BWD * dev_ncu());
  w.ks = cmlp_bwd_ksplit(C, HID);
  w.dw1_part = c.take<float>((size_t)w.grid * w.ks * HID * C);
  w.db1_part = c.take<float>((size_t)w.grid * 4 * HID);
  w.dw2_part = c.take<float>((size_t)w.grid * w.ks * C * HID);
  w.db2_part = c.take<float>((size_t)w.grid * 4 * C);
  w.dg_part = c.take<float>((size_t)w.grid * C);
  w.total = c.off;
  w.ok = c.ok;
  return w;
}
extern "C" size_t fno_channel_mlp_workspace_bytes(int C, int hidden, int B, size_t PW) {
  if (cmlp_check(B, C, hidden, PW) != FNO_OK) return 0;
  return carve_cmlp(C, hidden, B, PW, nullptr, 0).total;
}
template <int C, int HID>
static int cmlp_fwd_launch(hipStream_t st, const CmlpFwdArgs& a) {
  const size_t lds = cmlp_fwd_lds_bytes(C, HID);
  const int grid = std::min(a.ntiles, (2 * lds <= FNO_LDS_MAX ? 2 : 1) * dev_ncu());      // workgroups a CU holds
  return GT(1), LV(C == 32 ? "k_cmlp_fwd<32, 32>" : HID == 32 ? "k_cmlp_fwd<64, 32>" : "k_cmlp_fwd<64, 64>", 0, a.ntiles),
         launch("k_cmlp_fwd", k_cmlp_fwd<C, HID>, dim3(grid), dim3(256), lds, st, a);
}
template <int C, int HID>
static int cmlp_bwd_launch(hipStream_t st, int grid, const CmlpBwdArgs& a) {
  return GT(1), LV(C == 32 ? "k_cmlp_bwd<32, 32>" : HID == 32 ? "k_cmlp_bwd<64, 32>" : "k_cmlp_bwd<64, 64>", 0, a.ntiles),
         launch("k_cmlp_bwd", k_cmlp_bwd<C, HID>, dim3(grid), dim3(256), cmlp_bwd_lds_bytes(C, HID), st, a);
}
extern "C" int fno_channel_mlp_forward(int B, int C, int hidden, size_t PW, const float* u, const float* x, const float* w1,
                                       const float* b1, const float* w2, const float* b2, const float* gate, int gelu_out,
                                       float* y, void* stream) {
  LAUNCHCHK(cmlp_check(B, C, hidden, PW));
  if (!u || !x || !w1 || !b1 || !w2 || !b2 || !y) return fail(FNO_EINVAL, "fno_channel_mlp_forward: null argument");
  CmlpFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.g = gate; a.y = y; a.gelu_out = gelu_out ? 1 : 0;
  a.PW = (int)PW; a.tiles_per_plane = (int)(PW / 128); a.ntiles = B * a.tiles_per_plane;
  hipStream_t st = (hipStream_t)stream;
  if (C == 32) return cmlp_fwd_launch<32, 32>(st, a);
  return hidden == 32 ? cmlp_fwd_launch<64, 32>(st, a) : cmlp_fwd_launch<64, 64>(st, a);
}
extern "C" int fno_channel_mlp_backward(int B, int C, int hidden, size_t PW, const float* u, const float* x, const float* w1,
                                        const float* b1, const float* w2, const float* b2, const float* gate, int gelu_out,
                                        const float* dy, float* du, float* dx, float* dw1, float* db1, float* dw2, float* db2,
                                        float* dgate, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(cmlp_check(B, C, hidden, PW));
  if (!u || !x || !w1 || !b1 || !w2 || !b2 || !dy || !du || !dw1 || !db1 || !dw2 || !db2 || !ws)
    return fail(FNO_EINVAL, "fno_channel_mlp_backward: null argument");
  if ((gate == nullptr) != (dgate == nullptr)) return fail(FNO_EINVAL, "fno_channel_mlp_backward: dgate is null iff gate is null");
  CmlpWs w = carve_cmlp(C, hidden, B, PW, ws, ws_bytes);
  if (!w.ok) return fail(FNO_ENOMEM, "workspace too small: need %zu, have %zu", w.total, ws_bytes);
  CmlpBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u; a.x = x; a.dy = dy; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.g = gate; a.du = du; a.dx = dx;
  a.dw1_part = w.dw1_part; a.db1_part = w.db1_part; a.dw2_part = w.dw2_part; a.db2_part = w.db2_part;
  a.dg_part = gate ? w.dg_part : nullptr;
  a.gelu_out = gelu_out ? 1 : 0;
  a.PW = (int)PW; a.tiles_per_plane = (int)(PW / 128); a.ntiles = B * a.tiles_per_plane;
  hipStream_t st = (hipStream_t)stream;
  if (C == 32) LAUNCHCHK((cmlp_bwd_launch<32, 32>(st, w.grid, a)));
  else LAUNCHCHK((hidden == 32 ? cmlp_bwd_launch<64, 32>(st, w.grid, a) : cmlp_bwd_launch<64, 64>(st, w.grid, a)));
  JobList jobs;
  jobs.add(w.dw1_part, dw1, w.grid * w.ks, hidden, C, C, C);
  jobs.add(w.db1_part, db1, w.grid * 4, 1, hidden, hidden, hidden);
  jobs.add(w.dw2_part, dw2, w.grid * w.ks, C, hidden, hidden, hidden);
  jobs.add(w.db2_part, db2, w.grid * 4, 1, C, C, C);
  if (gate) jobs.add(w.dg_part, dgate, w.grid, 1, C, C, C);
  return jobs.run(st);
}

// ===========================================================================
// Domain padding (neuralop/models/padding.py:35-95; k_domain_pad.h): zero-pad a (planes, dims) tensor, or crop the interior
// back out.  One launch either way, laid over the output in 16-byte quads.
// ===========================================================================
static constexpr int FNO_GRID_DOMPAD = 8;                     // workgroups of 256 threads a CU holds (four waves each, no LDS)
static constexpr long long DOMPAD_MAX_EXTENT = 1ll << 30;      // per padded axis: coordinates and their sums stay in int
static constexpr long long DOMPAD_MAX_ELEMS = 1ll << 62;       // in all: flat offsets stay in a signed 64-bit integer
static int dompad_run(bool pad, const char* fn, int ndim, size_t planes, const int* dims, const int* before, const int* after,
                      const float* src, float* dst, void* stream) {
  if (!dims || !before || !after || !src || !dst) return fail(FNO_EINVAL, "%s: null argument", fn);
  if (ndim < 1 || ndim > 3) return fail(FNO_EINVAL, "%s: ndim=%d (1, 2 or 3)", fn, ndim);
  long long U[3] = {1, 1, 1}, P[3] = {1, 1, 1}, bf[3] = {0, 0, 0};      // unpadded, padded, leading zeros; right-aligned
  for (int d = 0; d < ndim; ++d) {
    const int k = 3 - ndim + d;
    if (dims[d] < 1) return fail(FNO_EINVAL, "%s: dims[%d]=%d (at least 1)", fn, d, dims[d]);
    if (before[d] < 0 || after[d] < 0) return fail(FNO_EINVAL, "%s: negative pad on axis %d (before %d, after %d)", fn, d, before[d], after[d]);
    U[k] = dims[d];
    bf[k] = before[d];
    P[k] = (long long)dims[d] + before[d] + after[d];
  }
  long long total = (long long)std::min<size_t>(planes, (size_t)DOMPAD_MAX_ELEMS + 1);
  bool fits = total <= DOMPAD_MAX_ELEMS;
  for (int k = 0; k < 3; ++k) {
    fits = fits && P[k] <= DOMPAD_MAX_EXTENT && (total == 0 || P[k] <= DOMPAD_MAX_ELEMS / total);
    if (fits) total *= P[k];
  }
  if (!fits)
    return fail(FNO_EUNSUPPORTED, "%s: at most 2^30 elements per padded axis and 2^62 in the padded tensor (got %zu planes of %lld x %lld x %lld)",
                fn, planes, P[0], P[1], P[2]);
  if ((((uintptr_t)src | (uintptr_t)dst) & 3)) return fail(FNO_EINVAL, "%s: tensor not aligned to 4 bytes", fn);
  DomPadArgs a;
  memset(&a, 0, sizeof(a));
  a.in = (const unsigned*)src;
  a.out = (unsigned*)dst;
  for (int k = 0; k < 3; ++k) {
    a.R[k] = (int)(pad ? P[k] : U[k]);
    a.I[k] = (int)(pad ? U[k] : P[k]);
    a.off[k] = (int)(pad ? -bf[k] : bf[k]);
  }
  a.n_out = (long long)planes * a.R[0] * a.R[1] * a.R[2];
  if (a.n_out == 0) return FNO_OK;
  a.head = (int)std::min<long long>(a.n_out, (4 - (long long)(((uintptr_t)dst >> 2) & 3)) & 3);
  a.nq = (a.n_out - a.head) / 4;
  const long long blocks = std::max<long long>(1, std::min<long long>((a.nq + 255) / 256, (long long)FNO_GRID_DOMPAD * dev_ncu()));
  long long step = 4 * blocks * 256;
  for (int k = 2; k >= 0; --k) { a.s[k] = (int)(step % a.R[k]); step /= a.R[k]; }
  a.sp = step;
  const int nq = (int)std::min<long long>(a.nq, 0x7fffffff);
  if (pad) return LV("k_domain_pad", 0, nq), launch("k_domain_pad", k_domain_pad, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return LV("k_domain_crop", 0, nq), launch("k_domain_crop", k_domain_crop, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
}
extern "C" int fno_domain_pad(int ndim, size_t planes, const int* dims, const int* before, const int* after, const float* x,
                              float* y, void* stream) {
  return dompad_run(true, "fno_domain_pad", ndim, planes, dims, before, after, x, y, stream);
}
extern "C" int fno_domain_crop(int ndim, size_t planes, const int* dims, const int* before, const int* after, const float* y,
                               float* x, void* stream) {
  return dompad_run(false, "fno_domain_crop", ndim, planes, dims, before, after, y, x, stream);
}

// ===========================================================================
// Device-resident training data (k_data_gather.h): one strided (rows, cols) view of `count` snapshots picked by index from a
// pool, normalised (or only cast) and written as float32 planes `out_stride` floats apart.  One launch.
// ===========================================================================
template <typename S, bool NORM>
static int data_gather_launch(const char* tag, int stat_dtype, dim3 grid, hipStream_t st, const DataGatherArgs& a) {
  LV(tag, 0, (int)std::min<unsigned long long>(a.count, 0x7fffffffull));
  if constexpr (NORM) {      // (the cast-only kernels read no statistics: one instantiation per snapshot type)
    if (stat_dtype == 1) return launch("k_data_gather", k_data_gather<S, double, true>, grid, dim3(256), 0, st, a);
  }
  return launch("k_data_gather", k_data_gather<S, float, NORM>, grid, dim3(256), 0, st, a);
}
extern "C" int fno_data_gather(int src_dtype, int stat_dtype, const void* src, size_t n_src, size_t snap_elems, size_t offset,
                               size_t row_stride, size_t col_stride, int rows, int cols, const long long* idx, size_t count,
                               const void* mean, const void* std_, double eps, float* out, size_t out_stride, void* stream) {
  const char* fn = "fno_data_gather";
  if (!src || !idx || !out) return fail(FNO_EINVAL, "%s: null argument", fn);
  if (!mean != !std_) return fail(FNO_EINVAL, "%s: mean and std_ are given together or both NULL", fn);
  const bool norm = mean != nullptr;
  if (src_dtype < 0 || src_dtype > 1) return fail(FNO_EINVAL, "%s: src_dtype=%d (0 = float32, 1 = float64)", fn, src_dtype);
  if (norm && (stat_dtype < 0 || stat_dtype > 1)) return fail(FNO_EINVAL, "%s: stat_dtype=%d (0 = float32, 1 = float64)", fn, stat_dtype);
  if (rows < 1 || cols < 1) return fail(FNO_EINVAL, "%s: a view of %d x %d elements (at least 1 x 1)", fn, rows, cols);
  const unsigned long long n = (unsigned long long)rows * (unsigned long long)cols;
  if (out_stride < n) return fail(FNO_EINVAL, "%s: out_stride %zu is shorter than the %d x %d plane", fn, out_stride, rows, cols);
  const unsigned __int128 last = (unsigned __int128)offset + (unsigned __int128)(rows - 1) * row_stride + (unsigned __int128)(cols - 1) * col_stride;
  if (last >= snap_elems)
    return fail(FNO_EINVAL, "%s: the view (offset %zu, %d rows %zu apart, %d columns %zu apart) leaves a snapshot of %zu elements", fn, offset,
                rows, row_stride, cols, col_stride, snap_elems);
  const size_t ssz = src_dtype ? 8 : 4, msz = stat_dtype ? 8 : 4;
  if ((unsigned __int128)n_src * snap_elems * ssz > ((unsigned __int128)1 << 62) || (unsigned __int128)count * out_stride > ((unsigned __int128)1 << 60))
    return fail(FNO_EUNSUPPORTED, "%s: at most 2^62 bytes in the pool and 2^60 floats in the output", fn);
  if (((uintptr_t)src & (ssz - 1)) || ((uintptr_t)idx & 7) || ((uintptr_t)out & 3) || (norm && (((uintptr_t)mean | (uintptr_t)std_) & (msz - 1))))
    return fail(FNO_EINVAL, "%s: tensor not aligned to its element size", fn);
  if (count == 0) return FNO_OK;
  DataGatherArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.idx = idx; a.mean = mean; a.sd = std_; a.out = out;
  a.n_src = n_src; a.snap_elems = snap_elems; a.offset = offset; a.row_stride = row_stride; a.col_stride = col_stride;
  a.out_stride = out_stride; a.count = count; a.n = (long long)n; a.cols = cols; a.eps = eps;
  const dim3 grid((unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((n / 4 + 255) / 256, 1024)),
                  (unsigned)std::min<size_t>(count, 65535));
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == 1) return norm ? data_gather_launch<double, true>("k_data_gather<f64, norm>", stat_dtype, grid, st, a)
                                  : data_gather_launch<double, false>("k_data_gather<f64, cast>", 0, grid, st, a);
  return norm ? data_gather_launch<float, true>("k_data_gather<f32, norm>", stat_dtype, grid, st, a)
              : data_gather_launch<float, false>("k_data_gather<f32, cast>", 0, grid, st, a);
}

// ===========================================================================
// Device-resident PINO training data (k_pino_batch.h): a batch of a MultipleReynoldsKFaDataset from its resident tensors, one
// launch per tensor: u as a transposing gather, a_in = (x, y, t, u0) written in place.
// ===========================================================================
extern "C" int fno_data_transpose_gather(const float* src, size_t n_src, int rows, int cols, const long long* idx, size_t count,
                                         float* out, size_t out_stride, void* stream) {
  const char* fn = "fno_data_transpose_gather";
  if (!src || !idx || !out) return fail(FNO_EINVAL, "%s: null argument", fn);
  if (rows < 1 || cols < 1) return fail(FNO_EINVAL, "%s: entries of %d x %d elements (at least 1 x 1)", fn, rows, cols);
  const unsigned long long n = (unsigned long long)rows * (unsigned long long)cols;
  if (out_stride < n) return fail(FNO_EINVAL, "%s: out_stride %zu is shorter than the %d x %d entry", fn, out_stride, rows, cols);
  if ((unsigned __int128)n_src * n * 4 > ((unsigned __int128)1 << 62) || (unsigned __int128)count * out_stride > ((unsigned __int128)1 << 60))
    return fail(FNO_EUNSUPPORTED, "%s: at most 2^62 bytes in the pool and 2^60 floats in the output", fn);
  if (((uintptr_t)src & 3) || ((uintptr_t)idx & 7) || ((uintptr_t)out & 3)) return fail(FNO_EINVAL, "%s: tensor not aligned to its element size", fn);
  if (count == 0) return FNO_OK;
  TransposeGatherArgs a;
  memset(&a, 0, sizeof(a));
  a.src = reinterpret_cast<const unsigned*>(src); a.idx = idx; a.out = reinterpret_cast<unsigned*>(out);
  a.n_src = n_src; a.out_stride = out_stride; a.count = count; a.rows = rows; a.cols = cols;
  const dim3 grid((unsigned)((cols + TG_COLS - 1) / TG_COLS), (unsigned)std::min<size_t>(count, 65535));
  LV(rows > TG_ROWS ? "k_data_transpose_gather<chunked>" : "k_data_transpose_gather<one tile>", 0, (int)std::min<size_t>(count, 0x7fffffff));
  return launch("k_data_transpose_gather", k_data_transpose_gather, grid, dim3(256), 0, (hipStream_t)stream, a);
}

extern "C" int fno_pino_input(const float* a0, size_t n_src, const long long* idx, size_t count, const float* gx, const float* gy,
                              const float* gt, int s1, int s2, int t, float* out, void* stream) {
  const char* fn = "fno_pino_input";
  if (!a0 || !idx || !gx || !gy || !gt || !out) return fail(FNO_EINVAL, "%s: null argument", fn);
  if (s1 < 1 || s2 < 1 || t < 1) return fail(FNO_EINVAL, "%s: a grid of %d x %d x %d points (at least 1 x 1 x 1)", fn, s1, s2, t);
  const unsigned long long npts = (unsigned long long)s1 * (unsigned long long)s2;
  if ((unsigned __int128)n_src * npts * 4 > ((unsigned __int128)1 << 62) || (unsigned __int128)count * npts * t * 4 > ((unsigned __int128)1 << 60))
    return fail(FNO_EUNSUPPORTED, "%s: at most 2^62 bytes in the pool and 2^60 floats in the output", fn);
  if (((uintptr_t)a0 & 3) || ((uintptr_t)idx & 7) || (((uintptr_t)gx | (uintptr_t)gy | (uintptr_t)gt) & 3))
    return fail(FNO_EINVAL, "%s: tensor not aligned to its element size", fn);
  if ((uintptr_t)out & 15) return fail(FNO_EINVAL, "%s: out must be aligned to 16 bytes (one store per grid point)", fn);
  if (count == 0) return FNO_OK;
  PinoInputArgs a;
  memset(&a, 0, sizeof(a));
  a.a0 = reinterpret_cast<const unsigned*>(a0); a.idx = idx; a.out = reinterpret_cast<unsigned*>(out);
  a.gx = reinterpret_cast<const unsigned*>(gx); a.gy = reinterpret_cast<const unsigned*>(gy); a.gt = reinterpret_cast<const unsigned*>(gt);
  a.n_src = n_src; a.count = count; a.npts = npts; a.s2 = s2; a.t = t;
  const dim3 grid((unsigned)std::min<unsigned long long>((npts + PIN_POINTS - 1) / PIN_POINTS, 1u << 20), (unsigned)std::min<size_t>(count, 65535));
  LV("k_pino_input", 0, (int)std::min<size_t>(count, 0x7fffffff));
  return launch("k_pino_input", k_pino_input, grid, dim3(256), 0, (hipStream_t)stream, a);
}

// ===========================================================================
// Lifting layer on its own:  y = W x + b,  x (B, Cin <= 4, PW) -> y (B, C, PW), and its parameter gradients.
// (neuralop/models/tfno.py:11-20; the composed fc0 + Re-conditioning front of the PINO observers.)
// ===========================================================================
static int lift_check(int B, int Cin, int C, size_t PW) {
  LAUNCHCHK(pw_check(B, C, PW));
  if (Cin < 1 || Cin > 4) return fail(FNO_EUNSUPPORTED, "lifting: 1..4 input channels (got %d)", Cin);
  return FNO_OK;
}
extern "C" size_t fno_lifting_workspace_bytes(int C) { return (size_t)3 * dev_ncu() * C * 16 * sizeof(float) + 256; }
extern "C" int fno_lifting_forward(int B, int Cin, int C, size_t PW, const float* x, const float* w, const float* bias,
                                   float* y, void* stream) {
  LAUNCHCHK(lift_check(B, Cin, C, PW));
  if (!x || !w || !y) return fail(FNO_EINVAL, "fno_lifting_forward: null argument");
  PwShell p(C);
  p.d.Cin = Cin;
  PwFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.bias = bias; a.u = y;
  a.PW = (int)PW; a.W = 128; a.P = (int)(PW / 128);
  a.tiles_per_plane = (int)(PW / 128); a.ntiles = B * a.tiles_per_plane;
  return launch_lift(&p, (hipStream_t)stream, std::min(a.ntiles, FNO_GRID_LIFT * p.ncu), a);
}
extern "C" int fno_lifting_backward(int B, int Cin, int C, size_t PW, const float* x, const float* dy, float* dw,
                                    float* dbias, void* ws, size_t ws_bytes, void* stream) {
  LAUNCHCHK(lift_check(B, Cin, C, PW));
  if (!x || !dy || !dw || !ws) return fail(FNO_EINVAL, "fno_lifting_backward: null argument");
  if (ws_bytes < fno_lifting_workspace_bytes(C)) return fail(FNO_ENOMEM, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  LiftBwdArgs a;
  a.dy = dy; a.xin = x; a.dwl_part = (float*)ws; a.CL = Cin; a.PW = (int)PW;
  a.tiles_per_plane = (int)(PW / 128); a.ntiles = B * a.tiles_per_plane;
  const int grid = std::min(a.ntiles, 3 * dev_ncu());
  const size_t lds = ((size_t)C * 132 + 8 * 132) * 4;
  if (C == 32) LAUNCHCHK(launch("k_lift_bwd", k_lift_bwd<32, 128>, dim3(grid), dim3(256), lds, st, a));
  else LAUNCHCHK(launch("k_lift_bwd", k_lift_bwd<64, 128>, dim3(grid), dim3(256), lds, st, a));
  JobList jobs;
  jobs.add(a.dwl_part, dw, grid, C, Cin, 16, Cin);
  if (dbias) jobs.add(a.dwl_part + Cin, dbias, grid, C, 1, 16, 1);
  return jobs.run(st);
}
// dx[b][k][px] = sum_c w[c][k] dy[b][c][px], channels ascending: the lifting's adjoint on its own (k_lift_dx, k_block_bwd.h)
extern "C" int fno_lifting_backward_dx(int B, int Cin, int C, size_t PW, const float* dy, const float* w, float* dx, void* stream) {
  LAUNCHCHK(lift_check(B, Cin, C, PW));
  if (!dy || !w || !dx) return fail(FNO_EINVAL, "fno_lifting_backward_dx: null argument");
  if ((((uintptr_t)dy | (uintptr_t)dx) & 15) || ((uintptr_t)w & 3)) return fail(FNO_EINVAL, "fno_lifting_backward_dx: misaligned tensor");
  const size_t n4 = (size_t)B * PW / 4;
  return launch("k_lift_dx", k_lift_dx, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream, dy, w,
                dx, C, Cin, PW, n4);
}
