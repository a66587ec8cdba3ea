// Specialised 5G LDPC flooding decoder, launch path and C ABI: which variant of a code's generated kernel a call needs, its
// compiled code object and entry on the device, grid and workspace, the launch; the conversion of the state image.
// The programs and why they exist: ldpc5g_jit_gen.cpp.  Their compilation and the code-object cache: ldpc5g_jit_rtc.cpp.
#include <cstring>
#include "ldpc5g.h"
#include "ldpc5g_jit_rtc.h"

namespace samd {
// the forms of a code's kernel: output form x rule x state
constexpr int kVariants = 12;
static int variant_slot(int rib, JitRule rule, int state) { return (rib ? 1 : 0) + 2 * (int)rule + (state ? 6 : 0); }

struct JitState {
  std::mutex mu;
  Compiled* variant[kVariants] = {};           // by variant_slot
  int fn_dev[kVariants];                       // the device fn_cache[i] belongs to
  hipFunction_t fn_cache[kVariants] = {};
  std::atomic<long> launches{0};               // decodes this handle ran on a specialised kernel
  JitState() { std::fill(fn_dev, fn_dev + kVariants, -1); }
};

static JitVariant jit_variant(int state) {
  JitVariant v;
  v.state = state;
#ifdef SAMD_DEV
  v.abl = (int)opt_int("SAMD_JIT_ABL", 0);       // parts of an iteration removed: wrong results, development builds only
#endif
  return v;
}

static Compiled* get_compiled(const samd_ldpc5g* h, int rib, JitRule rule, int state = 0) {
  JitState* st = h->jit_state;
  const int vi = variant_slot(rib, rule, state);
  {
    std::lock_guard<std::mutex> lk(st->mu);
    if (st->variant[vi]) return st->variant[vi];
  }
  JitProgram prog = jit_generate(h, rib ? 1 : 0, rule, true, jit_variant(state ? 1 : 0));
  if (prog.source.empty()) {                                   // no such variant for this code (state: messages beyond LDS)
    static Compiled* const none = [] {
      Compiled* n = new Compiled();
      n->status = -1;
      n->log = "no generated kernel of this form for the code";
      return n;
    }();
    return none;
  }
  Compiled* c = jit_compile(std::move(prog), h->host_only != 0);
  std::lock_guard<std::mutex> lk(st->mu);
  st->variant[vi] = c;
  return c;
}

// the kernel's entry on the current device: the module is loaded once per (code object, device); a code object the device
// cannot load (another architecture, a runtime without the loader) is remembered as such and the caller runs the generic kernel
static hipFunction_t get_function(const samd_ldpc5g* h, Compiled* c, int vi, int dev) {
  JitState* st = h->jit_state;
  {
    std::lock_guard<std::mutex> lk(st->mu);
    if (st->fn_dev[vi] == dev) return st->fn_cache[vi];
  }
  hipFunction_t fn = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->fn.find(dev);
    if (it == c->fn.end()) {
      hipModule_t mod = nullptr;
      if (hipModuleLoadData(&mod, c->code.data()) != hipSuccess || hipModuleGetFunction(&fn, mod, c->prog.entry.c_str()) != hipSuccess) {
        (void)hipGetLastError();
        fn = nullptr;
        c->log += " (the code object did not load on device " + std::to_string(dev) + ")";
      }
      c->fn[dev] = fn;
    } else {
      fn = it->second;
    }
  }
  std::lock_guard<std::mutex> lk(st->mu);
  st->fn_dev[vi] = dev;
  st->fn_cache[vi] = fn;
  return fn;
}

// grid of the generated kernel for `batch` codewords (group codewords per workgroup, wgs workgroups per CU; 0: onchip_bp_grid)
static int jit_grid(const samd_ldpc5g* h, int batch, int group, int wgs) {
  if (wgs <= 0) return onchip_bp_grid(h, batch);
  const int ngroups = (batch + group - 1) / group;
  int grid = std::min(ngroups, device_cus() * wgs);
  if (h->opt.onchip_grid > 0) grid = std::min(grid, h->opt.onchip_grid);
  return grid;
}

size_t jit_workspace_bytes(const samd_ldpc5g* h, int batch, int cn_mode) {
  const JitRule rule = jit_rule(cn_mode);
  const bool phi = rule == JitRule::BoxplusPhi;                // (whose programs never spill: 0)
  if (!h || !h->jit_plan || h->opt.jit <= 0 || rule == JitRule::None || batch <= 0) return 0;
  if (jit_class(h, phi) != 2) return 0;
  JitGeometry g;
  if (!jit_geometry(h, phi, &g) || g.ws_bytes == 0) return 0;
  return (size_t)jit_grid(h, batch, g.pairx ? 2 * g.G : g.G, g.wgs) * g.ws_bytes + 256;
}

int launch_onchip_jit(const samd_ldpc5g* h, const float* llr, float* out, int batch, int num_iter, int cn_mode,
                      float llr_max, float offset, int hard_out, int return_infobits, void* workspace, size_t workspace_bytes,
                      void* stream, const float* state_in, float* state_out) {
  const JitRule rule = jit_rule(cn_mode);
  const bool phi = rule == JitRule::BoxplusPhi;
  const int with_state = (state_in || state_out) ? 1 : 0;
  if (!h->jit_state || h->opt.jit <= 0 || num_iter < 1 || rule == JitRule::None) return SAMD_ERR_UNSUPPORTED;
  {
    const int cls = jit_class(h, phi);
    if (!cls) return SAMD_ERR_UNSUPPORTED;
    if (phi && h->opt.jit_phi == 0) return SAMD_ERR_UNSUPPORTED;
    if (phi && h->opt.jit_phi < 0 && cls == 2) {        // default: not where one codeword leaves lanes of its only chunk idle
      JitGeometry g;
      if (!jit_geometry(h, true, &g) || (g.G == 1 && g.P % 64 != 0)) return SAMD_ERR_UNSUPPORTED;
    }
    if (phi && cls == 1 && (size_t)h->jit_plan->edges * h->z * 4 + 512 > 160 * 1024) return SAMD_ERR_UNSUPPORTED;
  }
  if (h->opt.jit == 1 && batch < h->opt.jit_min_batch && !with_state) return SAMD_ERR_UNSUPPORTED;
  const int rib = return_infobits ? 1 : 0;
  Compiled* c = get_compiled(h, rib, rule, with_state);
  if (c->status != 1) {
    set_error("specialised LDPC kernel unavailable: " + c->log);
    return SAMD_ERR_UNSUPPORTED;
  }
  int dev = 0;
  SAMD_HIP_CHECK(hipGetDevice(&dev));
  hipFunction_t fn = get_function(h, c, variant_slot(rib, rule, with_state), dev);
  if (!fn) {
    set_error("specialised LDPC kernel unavailable: " + c->log);
    return SAMD_ERR_UNSUPPORTED;
  }
  float off = (cn_mode == SAMD_CN_OFFSET_MINSUM) ? offset : 0.f;
  const int grid = jit_grid(h, batch, c->prog.group, c->prog.wgs);
  float* ws = nullptr;
  if (c->prog.ws_bytes) {                                           // the last base rows' messages: a row per workgroup, caller-owned
    const size_t need = (size_t)grid * c->prog.ws_bytes + 256;
    if (!workspace || workspace_bytes < need) {
      set_error("workspace too small (samd_ldpc5g_decode_workspace_bytes)");
      return SAMD_ERR_WORKSPACE;
    }
    ws = reinterpret_cast<float*>(align_up((size_t)workspace, 256));
  }
  void* args[] = {(void*)&llr, (void*)&out, (void*)&batch, (void*)&num_iter, (void*)&llr_max, (void*)&off, (void*)&hard_out, (void*)&ws,
                  (void*)&state_in, (void*)&state_out};
  if (hipModuleLaunchKernel(fn, grid, 1, 1, 64 * (unsigned)c->prog.waves, 1, 1, 0, (hipStream_t)stream, args, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    set_error("specialised LDPC kernel: launch failed");
    return SAMD_ERR_UNSUPPORTED;                               // the caller's generic kernel takes the batch
  }
  h->jit_state->launches.fetch_add(1, std::memory_order_relaxed);
  return SAMD_OK;
}

JitState* new_jit_state() { return new JitState(); }

void free_jit(samd_ldpc5g* h) {
  delete h->jit_plan;
  h->jit_plan = nullptr;
  delete h->jit_state;          // compiled code stays in the process-wide cache
  h->jit_state = nullptr;
}

// image [passes][img] <-> canonical [num_edges][batch] (logit sign: the state the reference returns is -1 x the internal v2c,
// ldpc_bp_generic.hip state_copy_kernel).  A workgroup = 128 image floats x 64 passes through an LDS tile: the image side moves
// 512 contiguous bytes per pass, the canonical side 64 passes of one edge (256 bytes when a pass is one codeword).
__global__ __launch_bounds__(256) void state_convert_kernel(const int32_t* __restrict__ table, int img, int cwpp, long batch, float* __restrict__ image,
                                                            float* __restrict__ canon, int to_canon) {
  __shared__ float tile[64][129];
  const int q0 = blockIdx.x * 128, u0 = blockIdx.y * 64;
  const long passes = (batch + cwpp - 1) / cwpp;
  const int t = threadIdx.x;
  // one codeword per pass and a batch of whole float4s: the reference's side moves 16 bytes per lane (64 passes = 256 bytes
  // per edge as four lanes' float4 instead of 64 lanes' floats)
  const bool vec = cwpp == 1 && (batch & 3) == 0 && u0 + 64 <= passes;
  if (to_canon) {
    for (int i = t; i < 64 * 128; i += 256) {
      const int u = i >> 7, q = i & 127;
      tile[u][q] = (u0 + u < passes && q0 + q < img) ? image[(size_t)(u0 + u) * img + q0 + q] : 0.f;
    }
    __syncthreads();
    if (vec) {
      for (int i = t; i < 16 * 128; i += 256) {
        const int q = i >> 4, u = (i & 15) * 4;
        if (q0 + q >= img) continue;
        const int32_t te = table[q0 + q];
        if (te < 0) continue;
        *reinterpret_cast<float4*>(canon + (size_t)(te & 0xFFFFFF) * batch + u0 + u) =
            make_float4(-1.f * tile[u][q], -1.f * tile[u + 1][q], -1.f * tile[u + 2][q], -1.f * tile[u + 3][q]);
      }
      return;
    }
    for (int i = t; i < 64 * 128; i += 256) {
      const int q = i >> 6, u = i & 63;
      if (q0 + q >= img) continue;
      const int32_t te = table[q0 + q];
      if (te < 0) continue;
      const long b = (long)(u0 + u) * cwpp + (te >> 24);
      if (u0 + u < passes && b < batch) canon[(size_t)(te & 0xFFFFFF) * batch + b] = -1.f * tile[u][q];
    }
  } else {
    if (vec) {
      for (int i = t; i < 16 * 128; i += 256) {
        const int q = i >> 4, u = (i & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + q < img) {
          const int32_t te = table[q0 + q];
          if (te >= 0) v = *reinterpret_cast<const float4*>(canon + (size_t)(te & 0xFFFFFF) * batch + u0 + u);
        }
        tile[u][q] = -1.f * v.x; tile[u + 1][q] = -1.f * v.y; tile[u + 2][q] = -1.f * v.z; tile[u + 3][q] = -1.f * v.w;
      }
    } else
    for (int i = t; i < 64 * 128; i += 256) {
      const int q = i >> 6, u = i & 63;
      float v = 0.f;
      if (q0 + q < img) {
        const int32_t te = table[q0 + q];
        const long b = (long)(u0 + u) * cwpp + (te >> 24);
        if (te >= 0 && u0 + u < passes && b < batch) v = -1.f * canon[(size_t)(te & 0xFFFFFF) * batch + b];
      }
      tile[u][q] = v;
    }
    __syncthreads();
    for (int i = t; i < 64 * 128; i += 256) {
      const int u = i >> 7, q = i & 127;
      if (u0 + u < passes && q0 + q < img) image[(size_t)(u0 + u) * img + q0 + q] = tile[u][q];
    }
  }
}
}  // namespace samd

using namespace samd;

extern "C" int samd_ldpc5g_state_layout(const samd_ldpc5g_t* h, int cn_mode, int* img_floats, int* cw_per_pass) {
  JitProgram p;   // (of the state variant, which must exist: a partly filled only chunk has no whole wave to move the image)
  if (!jit_state_layout(h, jit_rule(cn_mode), &p)) { set_error("no generated kernel with state for this code / rule"); return SAMD_ERR_UNSUPPORTED; }
  if (img_floats) *img_floats = (int)(p.img_bytes / 4);
  if (cw_per_pass) *cw_per_pass = p.group;
  return SAMD_OK;
}

extern "C" int samd_ldpc5g_state_map(const samd_ldpc5g_t* h, int cn_mode, int32_t* cw, int32_t* cn, int32_t* vn) {
  SAMD_REQUIRE(h && cw && cn && vn, "null argument");
  const int rc = jit_state_map(h, jit_rule(cn_mode), cw, cn, vn);
  if (rc != SAMD_OK) set_error("no generated kernel with state for this code / rule");
  return rc;
}

extern "C" int samd_ldpc5g_state_convert_f32(const int32_t* table, int img_floats, int cw_per_pass, long batch, float* image,
                                             float* canonical, int to_canonical, void* stream) {
  SAMD_REQUIRE(table && image && canonical && img_floats > 0 && cw_per_pass > 0 && batch >= 0, "bad argument");
  if (batch == 0) return SAMD_OK;
  const long passes = (batch + cw_per_pass - 1) / cw_per_pass;
  const dim3 grid((unsigned)((img_floats + 127) / 128), (unsigned)((passes + 63) / 64));
  hipLaunchKernelGGL(state_convert_kernel, grid, dim3(256), 0, (hipStream_t)stream, table, img_floats, cw_per_pass, batch, image, canonical,
                     to_canonical);
  SAMD_HIP_CHECK(hipGetLastError());
  return SAMD_OK;
}

// LDPC5GDecoder.call with return_state / msg_v2c on the generated kernel: image_in (or null: start from the channel values),
// image_out (or null), both [ceil(batch / cw_per_pass)][img_floats] device floats in the layout of samd_ldpc5g_state_map
extern "C" int samd_ldpc5g_decode_state_f32(const samd_ldpc5g_t* h, const float* llr, float* out, const float* image_in, float* image_out,
                                            int batch, int num_iter, int cn_mode, float llr_max, float offset, int hard_out,
                                            int return_infobits, void* stream) {
  SAMD_REQUIRE(h && llr && out && (image_in || image_out), "null argument");
  if (batch <= 0) return SAMD_OK;
  return launch_onchip_jit(h, llr, out, batch, num_iter, cn_mode, llr_max, offset, hard_out, return_infobits, nullptr, 0, stream, image_in,
                           image_out);
}

// ---- C-ABI (include/sionna_amd.h)
extern "C" int samd_ldpc5g_jit_supported(const samd_ldpc5g_t* h) { return jit_eligible(h) ? 1 : 0; }

extern "C" long samd_ldpc5g_jit_source(const samd_ldpc5g_t* h, int return_infobits, int cn_mode, int with_ops, char* buf,
                                       size_t cap) {
  if (!jit_eligible(h)) { set_error("code outside the class of the specialised kernel"); return SAMD_ERR_UNSUPPORTED; }
  if (jit_rule(cn_mode) == JitRule::None) { set_error("no specialised kernel for this rule"); return SAMD_ERR_UNSUPPORTED; }
  // (SAMD_JIT_STATE = 1: the text of the state variant, for tools and tests/jit_emu)
  const std::string src = jit_generate(h, return_infobits ? 1 : 0, jit_rule(cn_mode), with_ops != 0, jit_variant((int)opt_int("SAMD_JIT_STATE", 0))).source;
  if (src.empty()) { set_error("no generated kernel of this form for the code"); return SAMD_ERR_UNSUPPORTED; }
  if (buf && cap > 0) {
    const size_t n = std::min(cap - 1, src.size());
    memcpy(buf, src.data(), n);
    buf[n] = 0;
  }
  return (long)src.size();
}

// compiles (or finds) the specialised kernel now instead of at the first large decode; 1 = ready, 0 = not in the class /
// switched off, < 0 = compilation failed (samd_last_error holds the compiler's log)
extern "C" int samd_ldpc5g_jit_prepare(const samd_ldpc5g_t* h, int return_infobits, int cn_mode) {
  if (!h || !h->jit_state || !jit_eligible(h) || h->opt.jit <= 0) return 0;
  if (jit_rule(cn_mode) == JitRule::None) return 0;
  Compiled* c = get_compiled(h, return_infobits ? 1 : 0, jit_rule(cn_mode));
  if (c->status != 1) { set_error("specialised LDPC kernel: " + c->log); return SAMD_ERR_HIP; }
  return 1;
}

// number of samd_ldpc5g_decode_f32 calls of this handle that ran on a specialised kernel (tests assert that the path
// they mean to exercise is the one that ran)
extern "C" long samd_ldpc5g_jit_launches(const samd_ldpc5g_t* h) {
  return (h && h->jit_state) ? h->jit_state->launches.load(std::memory_order_relaxed) : 0;
}

// process-wide counters of the code-object cache: what[0] = hipRTC compilations, what[1] = code objects read from disk
extern "C" int samd_ldpc5g_jit_cache_stats(long* what) {
  if (!what) return SAMD_ERR_INVALID;
  jit_compile_stats(what);
  return SAMD_OK;
}

// compiled code object of the specialised kernel (for disassembly / inspection); returns its size
extern "C" long samd_ldpc5g_jit_code(const samd_ldpc5g_t* h, int return_infobits, int cn_mode, char* buf, size_t cap) {
  if (samd_ldpc5g_jit_prepare(h, return_infobits, cn_mode) != 1) return SAMD_ERR_UNSUPPORTED;
  Compiled* c = get_compiled(h, return_infobits ? 1 : 0, jit_rule(cn_mode));
  if (buf && cap >= c->code.size()) memcpy(buf, c->code.data(), c->code.size());
  return (long)c->code.size();
}
