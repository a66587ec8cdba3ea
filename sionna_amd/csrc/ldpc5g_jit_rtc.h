// Run-time compilation of a generated program (ldpc5g_jit_rtc.cpp) as the launch path (ldpc5g_jit.cpp) sees it.
#pragma once
#include <map>
#include <mutex>

#include "common.h"
#include "ldpc5g_jit.h"

namespace samd {
// a compiled code object, shared by all handles whose program has the same text and target
struct Compiled {
  std::once_flag once;               // the compile (or the read of the cached code object) happens outside the map's lock
  int status = 0;                    // 1 ok, -1 failed
  std::string log, arch;
  std::vector<char> code;
  std::mutex mu;                     // fn
  std::map<int, hipFunction_t> fn;   // per device; nullptr: the module did not load there
  JitProgram prog;                   // what a launch must know, as the generator stated it (without the text: the cache's key)
};
// The code object of a program for the current device's architecture (host_only: the product's target), from the process-wide
// cache, the disk cache or hipRTC - compiled once per text and target, whoever asks first.  Never null; status tells.
Compiled* jit_compile(JitProgram&& prog, bool host_only);
// process-wide counters: what[0] = hipRTC compilations, what[1] = code objects read from disk
void jit_compile_stats(long* what);
}  // namespace samd
