// Every ECGMM_* environment switch the native code reads: name, parsing, default, run-time clamp and one line of meaning,
// in ONE table (the order of INTEGRATION.md section 5 and of ecgmm_switch_name()).  The measurements behind each default
// stay next to the code that reads the switch.  The env_* helpers of common.h are called from here only.
#pragma once
#include <limits.h>

#include "common.h"

struct Switch {
  enum Kind {
    ON,     // on unless the value starts with '0' (env_on)
    OFF,    // off unless the value starts with '1' (env_off)
    LEVEL,  // one digit 0..hi, anything else: the default (env_level); set() clamps to 0..hi
    INT     // an integer (env_int); a negative one, from the environment or set(), becomes `neg`
  };
  const char* env;
  Kind kind;
  long def;      // the value when the variable is unset
  long hi, neg;  // see Kind
  bool runtime;  // may change after start-up; false: ecgmm_switch_set refuses (what was read must keep holding)
  const char* doc;
  long v = LONG_MIN;  // LONG_MIN: not read yet

  long clamp(long x) const {
    if (kind == LEVEL) return x < 0 ? 0 : x > hi ? hi : x;
    if (kind == INT) return x < 0 ? neg : x;
    return x != 0;
  }
  long from_env() const {
    if (kind == ON) return env_on(env);
    if (kind == OFF) return env_off(env);
    if (kind == LEVEL) return env_level(env, (int)hi, (int)def);
    return clamp(env_int(env, def));
  }
  // the environment is read at the first get() unless a set() came first; afterwards one load and one compare
  long get() {
    if (v == LONG_MIN) v = from_env();
    return v;
  }
  void set(long x) { v = clamp(x); }
};

namespace sw {
constexpr long NEVER = 1L << 40;  // a pixel count no layer reaches
// clang-format off
//                       variable                  kind          def   hi neg   runtime
// ---- halo-resident convolution kernel (conv_halo.hip)
inline Switch CONV_HALO      {"ECGMM_CONV_HALO",       Switch::LEVEL, 1,     2, 0,     true,  "halo-resident conv kernel: 0 = never, 1 = where it is faster, 2 = wherever applicable"};
inline Switch HALO_CUS       {"ECGMM_HALO_CUS",        Switch::INT,   0,     0, 0,     true,  "cap on the CUs (persistent workgroups) of a halo-kernel launch; 0 or negative = all"};
inline Switch HALO_W4        {"ECGMM_HALO_W4",         Switch::OFF,   0,     0, 0,     true,  "64 -> 64 channel 3x3 tiles on 4-wave workgroups, two per CU"};
inline Switch HALO_STAGGER   {"ECGMM_HALO_STAGGER",    Switch::ON,    1,     0, 0,     true,  "waves 4-7 run a step's first MFMA block behind its barrier (0: lock step); bit-identical"};
inline Switch HALO_STREAM    {"ECGMM_HALO_STREAM",     Switch::ON,    1,     0, 0,     true,  "stream form of the 64 -> 64 channel 3x3 tiles (0: one tile at a time); bit-identical"};
inline Switch HALO_PP        {"ECGMM_HALO_PP",         Switch::ON,    1,     0, 0,     true,  "ping-pong K loop on the 128-channel 3x3 tiles (0: lock step); bit-identical"};
inline Switch HALO_NCS1      {"ECGMM_HALO_NCS1",       Switch::ON,    1,     0, 0,     false, "64-channel 3x3 layers prefetch the next tile's halo during the K loop"};
// ---- weight gradients (conv_wgrad.hip)
inline Switch WGRAD_RING     {"ECGMM_WGRAD_RING",      Switch::LEVEL, 1,     2, 0,     true,  "ring weight-gradient kernel: 0 = never, 1 = where it is faster, 2 = wherever applicable"};
inline Switch WGRAD_PP       {"ECGMM_WGRAD_PP",        Switch::OFF,   0,     0, 0,     true,  "ping-pong between the two wave groups of the ring weight gradient; bit-identical"};
inline Switch WGRAD_GROUPS   {"ECGMM_WGRAD_GROUPS",    Switch::OFF,   0,     0, 0,     false, "1 = 256-thread weight-gradient workgroups instead of two 4-wave groups sharing a slab tile"};
inline Switch WGRAD_WGS      {"ECGMM_WGRAD_WGS",       Switch::INT,   0,     0, 0,     false, "four-wave slots of a weight-gradient launch; 0 or negative = 512 alone, the plan's choice on the side stream"};
// ---- BatchNorm passes (elementwise.hip, plan_resnet18.hip)
inline Switch BN_FOLD        {"ECGMM_BN_FOLD",         Switch::ON,    1,     0, 0,     true,  "BatchNorm finalize folded into its consumer pass (0: separate launches)"};
inline Switch BN_FOLD_SLICE  {"ECGMM_BN_FOLD_SLICE",   Switch::ON,    1,     0, 0,     true,  "folded passes at C >= 256 as (pixel chunk, 128-channel slice) workgroups; bit-identical"};
inline Switch BN_FUSE        {"ECGMM_BN_FUSE",         Switch::ON,    1,     0, 0,     false, "0 = BatchNorm-backward reductions always as their own pass, whatever the threshold"};
inline Switch BN_FUSE_MIN_M  {"ECGMM_BN_FUSE_MIN_M",   Switch::INT,   NEVER, 0, NEVER, true,  "pixel count from which a BatchNorm-backward reduction is fused into the producing dgrad; negative = never"};
inline Switch RELU_BITS      {"ECGMM_RELU_BITS",       Switch::ON,    1,     0, 0,     false, "bn2's backward reads the ReLU mask as bits the forward wrote (forward and backward must agree)"};
inline Switch STEM_FUSE      {"ECGMM_STEM_FUSE",       Switch::ON,    1,     0, 0,     false, "stem backward as one pool + BatchNorm pass (0: max-pool backward + full BatchNorm backward)"};
// ---- encoder plans
inline Switch STEM_RECOMPUTE {"ECGMM_STEM_RECOMPUTE",  Switch::OFF,   0,     0, 0,     true,  "image stem by recompute, without its full-resolution conv output (changes the workspace layouts)"};
inline Switch DOWN_FOLD      {"ECGMM_DOWN_FOLD",       Switch::ON,    1,     0, 0,     false, "downsample branch's input gradient folded into the stride-2 dgrad (0: own launch + addend)"};
inline Switch DOWN_SIDE      {"ECGMM_DOWN_SIDE",       Switch::ON,    1,     0, 0,     false, "downsample branch of the training forward on the side stream (0: the caller's stream)"};
inline Switch SIDE_WGRAD     {"ECGMM_SIDE_WGRAD",      Switch::ON,    1,     0, 0,     false, "initial state of each plan's weight-gradient side stream; per plan at run time: ecgmm_side_wgrad()"};
inline Switch INFER_DOWN_SIDE{"ECGMM_INFER_DOWN_SIDE", Switch::OFF,   0,     0, 0,     true,  "downsample convolution of the inference plans on a side stream beside conv1"};
inline Switch SE_MERGE       {"ECGMM_SE_MERGE",        Switch::ON,    1,     0, 0,     false, "ResNet1D_SE backward: SE-gate gradient and bn2's reduction in one pass (0: two passes)"};
// ---- dense tails (head_fused.hip, linear.hip)
inline Switch SE_MLP_FUSED   {"ECGMM_SE_MLP_FUSED",    Switch::ON,    1,     0, 0,     false, "the SE MLP as fused kernels (0: per-op launches)"};
inline Switch HEAD_FUSED     {"ECGMM_HEAD_FUSED",      Switch::ON,    1,     0, 0,     false, "fusion head on the row kernels of head_fused.hip (0: ~45 per-op launches)"};
inline Switch DENSE16        {"ECGMM_DENSE16",         Switch::ON,    1,     0, 0,     false, "batch-sized Linear layers on dense16_kernel (0: the implicit-GEMM route)"};
// clang-format on

inline Switch* const ALL[] = {
    &CONV_HALO,  &HALO_CUS,      &HALO_W4,       &HALO_STAGGER, &HALO_STREAM,   &HALO_PP,   &HALO_NCS1,  &WGRAD_RING,      &WGRAD_PP,
    &WGRAD_GROUPS, &WGRAD_WGS,   &BN_FOLD,       &BN_FOLD_SLICE, &BN_FUSE,      &BN_FUSE_MIN_M, &RELU_BITS, &STEM_FUSE,    &STEM_RECOMPUTE,
    &DOWN_FOLD,  &DOWN_SIDE,     &SIDE_WGRAD,    &INFER_DOWN_SIDE, &SE_MERGE,   &SE_MLP_FUSED, &HEAD_FUSED, &DENSE16};
constexpr int COUNT = (int)(sizeof(ALL) / sizeof(ALL[0]));

inline Switch* find(const char* env) {
  for (Switch* s : ALL)
    if (env && strcmp(s->env, env) == 0) return s;
  return nullptr;
}
}  // namespace sw
