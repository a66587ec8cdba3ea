// Specialised 5G LDPC decoders: the per-wave work lists of the explicit-message engine (ldpc5g_onchip_bp.hip builds
// them, ldpc5g_decode_msg_kernel walks them with scalar code) turned into straight-line source for ONE code and
// compiled at run time with hipRTC for gfx950 (ldpc5g_jit_gen.cpp writes the text, ldpc5g_jit_rtc.cpp compiles it,
// ldpc5g_jit.cpp launches it).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

struct samd_ldpc5g;

namespace samd {

struct JitItem {
  int idx;    // base row (check-node item) or base column (variable-node item)
  int q;      // first 64-lane chunk of lifted copies
  int nch;    // chunks covered (1 or 2)
  int prio;   // issue priority 0..3 (ldpc5g.h: item_priorities)
};

// Host-side description of the schedule (kept with the handle; nothing here lives on the device)
struct JitPlan {
  int z = 0, edges = 0, ncu = 0, nbu = 0;
  std::vector<int32_t> row_off;                                     // [ncu] byte offset of the row's first edge block
  std::vector<int> row_deg, fused_col;                              // [ncu]; fused degree-1 column or -1
  std::vector<std::vector<std::pair<int32_t, int32_t>>> col_edges;  // [nbu] (edge block byte offset, 4 shift), rows ascending
  std::vector<char> col_fused;                                      // [nbu]
  std::vector<std::vector<JitItem>> cn, vn;                         // [16 waves], in issue order
  // general = 1: built for any code by build_jit_plan_general (graph data only: the generator makes its own schedule)
  int general = 0;
  int prune_row = -1, prune_z0 = 0;   // base row whose lifted copies z >= prune_z0 the rate matching pruned (decoding.py:1344-1373)
};

// how the any-lifting-size programs map lifted copies onto lanes (jit/ldpc5g_jit_templates.h, JIT_GENERAL)
struct JitGeometry {
  int G = 1;        // codewords per workgroup (pairx: PAIRS of codewords)
  int pairx = 0;    // 1: a slot's two values are copy z of TWO codewords (2 g, 2 g + 1) - any Z, odd ones too, a rotation never
                    // swaps the pair (no selections in the variable-node phase); 0: copies (z, z + Z / 2) of ONE codeword
  int H = 0;        // the rotation's period in lanes: Z / 2 (a lane owns copies (z, z + H)), or Z with pairx
  int P = 0;        // G H lanes in use
  int chunks = 0;   // 64-lane chunks per edge block
  int blk = 0;      // bytes per edge block (512 per chunk)
  int nw = 16;      // waves per workgroup
  int wgs = 1;      // workgroups per CU
  // codes whose messages exceed LDS: the edge blocks of the base rows >= spill_row live in the workgroup's row of a
  // caller-owned workspace (L2); e_lds = edges whose blocks stay in LDS (all of them without spill)
  int spill_row = -1, e_lds = 0;
  size_t ws_bytes = 0;   // bytes of one workgroup's workspace row
};

struct JitState;

// which form of a code's kernel is generated.  Everything else about the programs - schedule, message layout, lane geometry,
// the form of each node update - follows from the code and the rule alone (ldpc5g_jit_gen.cpp).
struct JitVariant {
  int state = 0;   // takes / returns the message image of a workgroup pass (return_state / msg_v2c)
  int abl = 0;     // -DSAMD_DEV builds: SAMD_JIT_ABL, parts of an iteration removed (see jit/ldpc5g_jit_templates.h)
};

// rule of a generated kernel (the values are part of the variant index); boxplus-phi on the defined exp / log
enum class JitRule { None = -1, OffsetMinSum = 0, MinSum = 1, BoxplusPhi = 2 };
JitRule jit_rule(int cn_mode);   // the one mapping from SAMD_CN_*; None: no generated kernel for the rule

// What the generator hands the runtime: the translation unit for hipRTC and, as data, what a launch must know about it.  The
// text carries the same numbers as `// JIT_*` comment lines for tests and tools; nothing reads them back.
struct JitProgram {
  std::string source;      // empty: no such variant for the code
  std::string entry;       // the kernel's name
  int waves = 0;           // workgroup size / 64
  int group = 1;           // codewords a workgroup decodes in one pass
  int wgs = 0;             // workgroups per CU (0: the grid of onchip_bp_grid)
  size_t ws_bytes = 0;     // workspace row of one workgroup (0: the messages fit LDS)
  unsigned img_bytes = 0;  // state variant: bytes of the message image of one workgroup pass ...
  unsigned img_msg0 = 0;   // ... and where it starts in LDS
  bool layout_b = false;   // the two chunks of an edge block interleaved (jit/ldpc5g_jit_templates.h: JIT_LAYOUT_B)
};

// ---- the generator (ldpc5g_jit_gen.cpp): host code, functions of the code and the rule alone
// true when the code is in the class the generator covers
bool jit_eligible(const samd_ldpc5g* h);
// with_ops = false: without the gfx950 operation definitions and the __global__ entry (what tests/jit_emu compiles for the CPU)
JitProgram jit_generate(const samd_ldpc5g* h, int return_infobits, JitRule rule, bool with_ops, JitVariant variant);
// the state variant's image: img_bytes, group and layout_b as jit_generate fills them, without the text (g: the lane geometry
// of class 2).  Returns the class; 0: no such variant
int jit_state_layout(const samd_ldpc5g* h, JitRule rule, JitProgram* p, JitGeometry* g = nullptr);
// per float of that image: codeword of the pass, check node, variable node (-1: the slot carries no edge); SAMD_OK or an error
int jit_state_map(const samd_ldpc5g* h, JitRule rule, int32_t* cw, int32_t* cn, int32_t* vn);
// graph data of the generator for a code that build_onchip_bp_tables left without a plan (any even lifting size)
void build_jit_plan_general(samd_ldpc5g* h, const std::vector<std::vector<std::pair<int, int>>>& by_row);
// 0: no generated kernel; 1: the Z = 128 k class (whole chunks of one kind, constants); 2: any-lifting-size programs
int jit_class(const samd_ldpc5g* h, bool phi);
bool jit_geometry(const samd_ldpc5g* h, bool phi, JitGeometry* g);

// ---- the launch path (ldpc5g_jit.cpp)
// SAMD_OK, SAMD_ERR_UNSUPPORTED (caller runs the generic kernel) or an error
int launch_onchip_jit(const samd_ldpc5g* h, const float* llr, float* out, int batch, int num_iter, int cn_mode,
                      float llr_max, float offset, int hard_out, int return_infobits, void* workspace, size_t workspace_bytes,
                      void* stream, const float* state_in = nullptr, float* state_out = nullptr);
// workspace the generated kernel of this code needs for `batch` codewords (0: none - the messages fit LDS - or no such kernel)
size_t jit_workspace_bytes(const samd_ldpc5g* h, int batch, int cn_mode);
JitState* new_jit_state();
void free_jit(samd_ldpc5g* h);

}  // namespace samd
