// Compiler binding and cache of the run-time compiled kernels: a program's text -> its code object for the current device,
// by hipRTC (bound lazily: the library loads without libhiprtc), kept per process and on disk.  Nothing here knows what the
// programs compute (ldpc5g_jit_gen.cpp writes them, ldpc5g_jit.cpp launches them).
#include "ldpc5g_jit_rtc.h"

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cstring>

#include "options.h"

namespace samd {
namespace {

typedef struct samd_hiprtc_prog_* rtc_prog;   // opaque (hiprtcProgram)
struct Rtc {
  void* lib = nullptr;
  int (*create)(rtc_prog*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
  int (*compile)(rtc_prog, int, const char* const*) = nullptr;
  int (*log_size)(rtc_prog, size_t*) = nullptr;
  int (*log)(rtc_prog, char*) = nullptr;
  int (*code_size)(rtc_prog, size_t*) = nullptr;
  int (*code)(rtc_prog, char*) = nullptr;
  int (*destroy)(rtc_prog*) = nullptr;
  int (*version)(int*, int*) = nullptr;
  bool ok = false;
  std::string ver = "?";
  Rtc() {
    for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return;
#define SAMD_RTC_SYM(field, sym) field = reinterpret_cast<decltype(field)>(dlsym(lib, sym))
    SAMD_RTC_SYM(create, "hiprtcCreateProgram");
    SAMD_RTC_SYM(compile, "hiprtcCompileProgram");
    SAMD_RTC_SYM(log_size, "hiprtcGetProgramLogSize");
    SAMD_RTC_SYM(log, "hiprtcGetProgramLog");
    SAMD_RTC_SYM(code_size, "hiprtcGetCodeSize");
    SAMD_RTC_SYM(code, "hiprtcGetCode");
    SAMD_RTC_SYM(destroy, "hiprtcDestroyProgram");
    SAMD_RTC_SYM(version, "hiprtcVersion");
#undef SAMD_RTC_SYM
    ok = create && compile && log_size && log && code_size && code && destroy;
    int ma = 0, mi = 0;
    if (version && version(&ma, &mi) == 0) ver = std::to_string(ma) + "." + std::to_string(mi);
  }
};
Rtc& rtc() {
  static Rtc r;
  return r;
}

// ---- SHA-256 (FIPS 180-4) of the cache key: source text + compiler version + target
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  unsigned char buf[64];
  size_t fill = 0;
  uint64_t total = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const unsigned char* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void update(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    total += n;
    while (n) {
      const size_t take = std::min(n, sizeof(buf) - fill);
      memcpy(buf + fill, p, take);
      fill += take; p += take; n -= take;
      if (fill == 64) { block(buf); fill = 0; }
    }
  }
  std::string hex() {
    const uint64_t bits = total * 8;
    const unsigned char one = 0x80, zero = 0;
    update(&one, 1);
    while (fill != 56) update(&zero, 1);
    unsigned char len[8];
    for (int i = 0; i < 8; ++i) len[i] = (unsigned char)(bits >> (56 - 8 * i));
    update(len, 8);
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return std::string(out, 64);
  }
};

// Code objects on disk: compiling a kernel takes ~4 s (hipRTC) in EVERY process - eight ranks x every (code, rule, output form)
// of a sweep.  <dir>/<sha256(source text | hipRTC version | target)>.co, dir = SAMD_JIT_CACHE_DIR, else
// $XDG_CACHE_HOME/sionna_amd, else $HOME/.cache/sionna_amd (both read once, at library load: api.cpp); SAMD_JIT_CACHE=0: off.
std::string cache_dir() {
  if (opt_int("SAMD_JIT_CACHE", 1) == 0) return std::string();
  std::string d = opt_str("SAMD_JIT_CACHE_DIR");
  if (d.empty()) {
    const std::string x = opt_str("SAMD__XDG_CACHE_HOME"), hm = opt_str("SAMD__HOME");
    if (!x.empty()) d = x + "/sionna_amd";
    else if (!hm.empty()) d = hm + "/.cache/sionna_amd";
  }
  return d;
}
void mkdirs(const std::string& path) {
  for (size_t i = 1; i <= path.size(); ++i)
    if (i == path.size() || path[i] == '/') (void)mkdir(path.substr(0, i).c_str(), 0755);
}
bool cache_read(const std::string& file, std::vector<char>* code) {
  FILE* f = fopen(file.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  bool ok = n > 64;
  if (ok) {
    code->resize((size_t)n);
    ok = fread(code->data(), 1, (size_t)n, f) == (size_t)n && memcmp(code->data(), "\x7f" "ELF", 4) == 0;
  }
  fclose(f);
  if (!ok) code->clear();
  return ok;
}
void cache_write(const std::string& dir, const std::string& file, const std::vector<char>& code) {
  mkdirs(dir);
  const std::string tmp = file + ".tmp." + std::to_string((long)getpid());
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return;
  const bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
  fclose(f);
  if (!ok || rename(tmp.c_str(), file.c_str()) != 0) (void)remove(tmp.c_str());   // rename: readers never see a partial file
}

// target of the code object: the architecture of the current device (the part of gcnArchName before the feature list);
// without a device (SAMD_HOST_ONLY tools) the product's target
std::string device_arch() {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.gcnArchName[0]) {
    std::string a = prop.gcnArchName;
    const size_t c = a.find(':');
    return c == std::string::npos ? a : a.substr(0, c);
  }
  (void)hipGetLastError();
  return "gfx950";
}

// compiled code objects, shared by all handles of the same code (target + source text is the key)
std::mutex g_mu;
std::map<std::string, Compiled*> g_cache;
std::atomic<long> g_compiles{0}, g_disk_hits{0};

int compile_source(const std::string& src, Compiled* c) {
  Rtc& r = rtc();
  const std::string dir = cache_dir();
  std::string file;
  if (!dir.empty()) {
    Sha256 sh;
    sh.update(src.data(), src.size());
    const std::string tail = "|hiprtc " + r.ver + "|" + c->arch;
    sh.update(tail.data(), tail.size());
    file = dir + "/" + sh.hex() + ".co";
    if (cache_read(file, &c->code)) { g_disk_hits.fetch_add(1); return 1; }
  }
  if (!r.ok) { c->log = "libhiprtc.so not available"; return -1; }
  rtc_prog p = nullptr;
  if (r.create(&p, src.c_str(), "samd_ldpc5g_jit.hip", 0, nullptr, nullptr) != 0) { c->log = "hiprtcCreateProgram failed"; return -1; }
  // -ffp-contract=off: the node updates restate the reference's arithmetic literally (as the library's Makefile does)
  const std::string arch_opt = "--offload-arch=" + c->arch;
  const char* opts[] = {arch_opt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off"};
  const int rc = r.compile(p, 4, opts);
  g_compiles.fetch_add(1);
  size_t ls = 0;
  if (r.log_size(p, &ls) == 0 && ls > 1) {
    c->log.resize(ls);
    r.log(p, &c->log[0]);
  }
  if (rc != 0) { r.destroy(&p); return -1; }
  size_t cs = 0;
  if (r.code_size(p, &cs) != 0 || cs == 0) { r.destroy(&p); c->log += " (no code)"; return -1; }
  c->code.resize(cs);
  const int gc = r.code(p, c->code.data());
  r.destroy(&p);
  if (gc != 0) return -1;
  if (!file.empty()) cache_write(dir, file, c->code);
  return 1;
}

}  // namespace

Compiled* jit_compile(JitProgram&& prog, bool host_only) {
  const std::string src = std::move(prog.source);
  const std::string arch = host_only ? std::string("gfx950") : device_arch();
  Compiled* c = nullptr;
  {
    std::lock_guard<std::mutex> gl(g_mu);
    Compiled*& slot = g_cache[arch + "|" + src];
    if (!slot) {
      slot = new Compiled();
      slot->arch = arch;
      slot->prog = std::move(prog);
      slot->prog.source.clear();
    }
    c = slot;
  }
  // compiling (or reading the cached code object) happens once per entry, outside g_mu: other codes and the launches of
  // kernels that exist already do not wait for it
  std::call_once(c->once, [&]() { c->status = compile_source(src, c); });
  return c;
}

void jit_compile_stats(long* what) {
  what[0] = g_compiles.load();
  what[1] = g_disk_hits.load();
}

}  // namespace samd
