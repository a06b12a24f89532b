// Custom-gate block of halo2's evaluate_h: an interpreter for GraphEvaluator programs (see gates.hip) and the straight-line
// kernels of the programs known ahead of time.  The host side -- the lowering, the tile rule, the program cache -- is
// gates_compile.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gates_compile.h"
#include "msm.h"

namespace sg {

// what a program known ahead of time may have for its columns and constants to travel as kernel arguments (GateArgsV in
// gates.hip, NumeratorArgs in numerator.h)
static constexpr uint32_t GATES_V_COLS = 24, GATES_V_CONSTS = 40;

// The development aids, read from the environment at every call (tests switch them between calls):
//   SG_GATES_GENERIC   every program runs in the interpreter          SG_GATES_DEBUG    one line per launch on stderr
//   SG_GATES_ROWS      the interpreter's rows per workgroup           SG_GATES_RELOAD, SG_GATES_CONVERT   GateLowering
struct GateEnv {
  bool generic, debug;
  uint32_t rows;
  GateLowering lowering;
};
GateEnv gates_env();

// a program the library has straight-line code for (the reference circuit's gate programs and its lookup input): launched with
// columns and constants as kernel arguments -- no blob; returns false (nothing launched) for any other program
bool gates_run_by_value(const GateProgram& p, const void* const* cols, fp_words* d_values, uint32_t k, uint32_t ext_k, hipStream_t stream,
                        uint32_t cosets, hipError_t* err);
// d_blob: [ops][column pointers][constants] as laid out by gates_blob(); values updated in place
size_t gates_blob(const GateProgram& p, const void* const* cols, std::vector<uint8_t>* blob);
// cosets = 0: arrays of 2^ext_k rows in halo2's extended-domain order; cosets = c: coset-major arrays of c * 2^k rows
hipError_t gates_run(const GateProgram& p, const uint8_t* d_blob, fp_words* d_values, uint32_t k, uint32_t ext_k,
                     hipStream_t stream, uint32_t cosets = 0);

}  // namespace sg
