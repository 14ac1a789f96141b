// Tile edge and k step of sgemm_f32.inc / sgemm_bf16x3.inc: the kernels and the hosts that size split-K partials by them
// (dcn_workspace.h) read the same two numbers.
#pragma once

namespace {

constexpr int SG_T = 128;        // tile edge
#ifndef SG_K_STEP
#define SG_K_STEP 16
#endif
constexpr int SG_K = SG_K_STEP;  // k per step

}  // namespace
