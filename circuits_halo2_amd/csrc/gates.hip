// Custom-gate block of the quotient numerator: values[row] <- program(row) for every
// row of the extended coset, where the program is halo2's GraphEvaluator (plonk/evaluation.rs of the
// pinned summa-dev/halo2 fork): a list of calculations over value sources (constants, earlier
// intermediates, fixed / advice / instance columns at a rotation, challenges, beta / gamma / theta / y,
// the previous value of the row).  halo2 runs it per row on the CPU with a Vec of intermediates; the
// circuit-specific part is the program, which the Rust side already holds, not this code.
//
// Host side (gates_compile.h: compile_gates, free of HIP): the graph is lowered to a straight-line program over LDS slots.
// Device side (gates_kernel): one thread per row, T rows per workgroup, slots in LDS as [slot][limb][row]
// (conflict-free), the instruction stream is uniform (scalar loads, no divergence).  Cost per
// product-type instruction ~260 VALU instructions (206 of them the product): ALU-bound like the rest.
#include "gates.h"
#include "gates_device.cuh"
#include "side_prio.cuh"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(gates_set_side_prio)

// ------------------------------------------------------------------ device

template <uint32_t T>
__global__ void __launch_bounds__(T) gates_kernel(GateArgs a) {
  side_kernel_prio();
  extern __shared__ uint32_t lds[];
  uint32_t* s_const = lds;                       // [n_consts][9]
  uint32_t* s_slot = lds + a.n_consts * 9;       // [n_slots][9][T]
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = tid; c < a.n_consts; c += T) {
    f29 v = f29_words_to_r261<P>(a.consts + 8 * c);
#pragma unroll
    for (int q = 0; q < 9; q++) s_const[c * 9 + q] = v.l[q];
  }
  __syncthreads();
  const size_t mask = (size_t)a.blockmask;
  const size_t row = (size_t)blockIdx.x * T + tid;
  if (row >= a.rows) return;
  const uint32_t rot_shift = a.ext_k - a.k;
  auto get = [&](uint32_t kind, uint32_t idx) {
    f29 r;
    if (kind == GK_CONST) {
#pragma unroll
      for (int q = 0; q < 9; q++) r.l[q] = s_const[idx * 9 + q];
    } else {
#pragma unroll
      for (int q = 0; q < 9; q++) r.l[q] = s_slot[(idx * 9 + q) * T + tid];
    }
    return r;
  };
  auto sub_k = [&](uint32_t kidx, const f29& x, const f29& y) {
    switch (kidx) {
      case 0: return gates_sub<P, 0>(x, y);
      case 1: return gates_sub<P, 1>(x, y);
      case 2: return gates_sub<P, 2>(x, y);
      case 3: return gates_sub<P, 3>(x, y);
      case 4: return gates_sub<P, 4>(x, y);
      default: return gates_sub<P, 5>(x, y);
    }
  };
  for (uint32_t pc = 0; pc < a.n_ops; pc++) {
    const GateOp op = a.ops[pc];
    const uint32_t code = op.w0 & 0xff, kidx = (op.w0 >> 8) & 0xff, ak = (op.w0 >> 16) & 0xff, bk = op.w0 >> 24;
    const uint32_t dst = op.dst & 0xffff;
    f29 r;
    switch (code) {
      case G_LOADCOL: {
        const size_t i = (row & ~mask) | ((row + ((size_t)(int64_t)(int32_t)op.b << rot_shift)) & mask);
        uint32_t w[8];
        fp_words_load(a.cols[op.a] + i, w);
        // kidx 0: memory words shifted left by 5 bits ARE the 2^261 form (bound 32), no product;
        // kidx 1: converted with one product (bound 2) -- for values with several consumers
        r = kidx ? f29_mul<P>(f29_from_words<0>(w), f29_const<P>(P::r266)) : f29_from_words<5>(w);
        break;
      }
      case G_LOADPREV: {
        uint32_t w[8];
        fp_words_load(a.values + row, w);
        r = f29_from_words<5>(w);
        break;
      }
      case G_ADD: r = f29_add(get(ak, op.a), get(bk, op.b)); break;
      case G_SUB: r = sub_k(kidx, get(ak, op.a), get(bk, op.b)); break;
      case G_MUL: r = f29_mul<P>(get(ak, op.a), get(bk, op.b)); break;
      case G_SQR: r = f29_sqr<P>(get(ak, op.a)); break;
      case G_DBL: { f29 x = get(ak, op.a); r = f29_add(x, x); break; }
      case G_NEG: r = sub_k(kidx, f29_zero(), get(ak, op.a)); break;
      case G_MULADD: r = f29_mul_add<P>(get(ak, op.a), get(bk, op.b), get(kidx, op.dst >> 16)); break;
      default: r = f29_reduce_small<P>(get(ak, op.a)); break;  // G_RED
    }
#pragma unroll
    for (int q = 0; q < 9; q++) s_slot[(dst * 9 + q) * T + tid] = r.l[q];
  }
  f29 res = get(a.result_kind, a.result_index);
  // hat -> memory domain: x^ * 2^256 * 2^-261 = x~, then canonical
  f29_store_canonical<P>(a.values + row, f29_mul<P>(res, f29_const<P>(P::r256)));
}

// A program known at compile time, for the rows of one workgroup: the constants are in LDS (2^261 domain), the result goes
// from the hat to the memory domain and is stored canonical.  The two kernels below differ in where the column pointers and the
// constants come from.
template <class PROG>
__device__ __forceinline__ void gates_fixed_rows(const fp_words* const* cols, fp_words* values, const uint32_t* s_const, uint64_t rows,
                                                 uint64_t blockmask, uint32_t rot_shift) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const GateSrc src{cols, values};
  const f29 res = gates_fixed_eval<PROG>(src, s_const, row, (size_t)blockmask, rot_shift);
  f29_store_canonical<P>(values + row, f29_mul<P>(res, f29_const<P>(P::r256)));
}

// columns and constants in the blob (gates_blob): any number of either
template <class PROG>
__global__ void __launch_bounds__(256) gates_fixed_kernel(GateArgs a) {
  side_kernel_prio();
  extern __shared__ uint32_t lds[];
  uint32_t* s_const = lds;                       // [n_consts][9]
  for (uint32_t c = threadIdx.x; c < a.n_consts; c += blockDim.x) {
    f29 v = f29_words_to_r261<P>(a.consts + 8 * c);
#pragma unroll
    for (int q = 0; q < 9; q++) s_const[c * 9 + q] = v.l[q];
  }
  __syncthreads();
  gates_fixed_rows<PROG>(a.cols, a.values, s_const, a.rows, a.blockmask, a.ext_k - a.k);
}

// the same with the column pointers and the constant table as kernel arguments: nothing to upload, nothing to keep alive
struct GateArgsV {
  fp_words* values;
  const fp_words* cols[GATES_V_COLS];
  uint32_t consts[GATES_V_CONSTS][8];
  uint32_t n_consts, k, ext_k;
  uint64_t rows, blockmask;
};
template <class PROG>
__global__ void __launch_bounds__(256) gates_fixed_value_kernel(GateArgsV a) {
  side_kernel_prio();
  __shared__ uint32_t s_const[GATES_V_CONSTS][9];
  if (threadIdx.x < a.n_consts) {
    const f29 v = f29_words_to_r261<P>(a.consts[threadIdx.x]);
#pragma unroll
    for (int q = 0; q < 9; q++) s_const[threadIdx.x][q] = v.l[q];
  }
  __syncthreads();
  gates_fixed_rows<PROG>(a.cols, a.values, &s_const[0][0], a.rows, a.blockmask, a.ext_k - a.k);
}

// ------------------------------------------------------------------ host: launches
GateEnv gates_env() {
  GateEnv e{};
  e.generic = std::getenv("SG_GATES_GENERIC") != nullptr;
  e.debug = std::getenv("SG_GATES_DEBUG") != nullptr;
  if (const char* v = std::getenv("SG_GATES_ROWS")) e.rows = (uint32_t)std::atoi(v);
  if (const char* v = std::getenv("SG_GATES_RELOAD")) e.lowering.reload_distance = (size_t)std::atoi(v);
  if (const char* v = std::getenv("SG_GATES_CONVERT")) {
    e.lowering.convert_at_load = true;
    e.lowering.convert_above = (uint32_t)std::atoi(v);
  }
  return e;
}

size_t gates_blob(const GateProgram& p, const void* const* cols, std::vector<uint8_t>* blob) {
  const size_t ops_b = p.ops.size() * sizeof(GateOp), cols_b = (size_t)p.n_columns * sizeof(void*),
               const_b = p.const_words.size() * sizeof(uint32_t);
  blob->resize(ops_b + cols_b + const_b + 16);
  std::memcpy(blob->data(), p.ops.data(), ops_b);
  if (cols_b) std::memcpy(blob->data() + ops_b, cols, cols_b);
  std::memcpy(blob->data() + ops_b + cols_b, p.const_words.data(), const_b);
  return blob->size();
}

// what both argument blocks say about the rows: cosets = 0: one block of 2^ext_k rows; cosets = c: c blocks of 2^k rows.
// Returns the number of rows.
template <class ARGS>
static size_t fill_rows(ARGS& a, const GateProgram& p, fp_words* d_values, uint32_t k, uint32_t ext_k, uint32_t cosets) {
  a.values = d_values;
  a.n_consts = (uint32_t)(p.const_words.size() / 8);
  a.k = k; a.ext_k = cosets ? k : ext_k;
  a.rows = cosets ? (size_t)cosets << k : (size_t)1 << ext_k;
  a.blockmask = ((uint64_t)1 << a.ext_k) - 1;
  return (size_t)a.rows;
}

bool gates_run_by_value(const GateProgram& p, const void* const* cols, fp_words* d_values, uint32_t k, uint32_t ext_k, hipStream_t stream,
                        uint32_t cosets, hipError_t* err) {
  *err = hipSuccess;
  const GateEnv env = gates_env();
  if (env.generic || p.n_columns > GATES_V_COLS || p.const_words.size() / 8 > GATES_V_CONSTS) return false;
  GateArgsV a;
  const unsigned blocks = (unsigned)((fill_rows(a, p, d_values, k, ext_k, cosets) + 255) / 256);
  for (uint32_t i = 0; i < p.n_columns; i++) a.cols[i] = static_cast<const fp_words*>(cols[i]);
  std::memcpy(a.consts, p.const_words.data(), p.const_words.size() * sizeof(uint32_t));
  const bool done = for_known_gate_program(p, [&](auto tag, const char* name) {
    if (env.debug) std::fprintf(stderr, "gates: ahead-of-time program %s (arguments by value), %u blocks\n", name, blocks);
    gates_fixed_value_kernel<decltype(tag)><<<blocks, 256, 0, stream>>>(a);
  });
  if (done) *err = hipGetLastError();
  return done;
}

template <uint32_t T>
static hipError_t launch_interpreter(const GateArgs& a, const GateTile& tile, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gates_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GATES_LDS_BUDGET);
  if (e != hipSuccess) return e;
  gates_kernel<T><<<(unsigned)((a.rows + T - 1) / T), T, tile.lds_bytes, stream>>>(a);
  return hipGetLastError();
}

hipError_t gates_run(const GateProgram& p, const uint8_t* d_blob, fp_words* d_values, uint32_t k, uint32_t ext_k,
                     hipStream_t stream, uint32_t cosets) {
  const GateEnv env = gates_env();
  GateArgs a;
  a.ops = reinterpret_cast<const GateOp*>(d_blob);
  a.cols = reinterpret_cast<const fp_words* const*>(d_blob + p.ops.size() * sizeof(GateOp));
  a.consts = reinterpret_cast<const uint32_t*>(d_blob + p.ops.size() * sizeof(GateOp) + (size_t)p.n_columns * sizeof(void*));
  a.n_ops = (uint32_t)p.ops.size();
  a.n_slots = p.n_slots;
  a.result_kind = p.result_kind;
  a.result_index = p.result_index;
  const size_t n_ext = fill_rows(a, p, d_values, k, ext_k, cosets);
  if (!env.generic) {   // a gate program known ahead of time: the straight-line kernel (any other program runs in the interpreter below)
    const unsigned blocks = (unsigned)((n_ext + 255) / 256);
    bool done = false;
    for_known_gate_program(p, [&](auto tag, const char* name) {
      using PROG = decltype(tag);
      if constexpr (is_circuit_gate_program<PROG>) {
        done = true;
        gates_fixed_kernel<PROG><<<blocks, 256, (size_t)a.n_consts * 36, stream>>>(a);
        if (env.debug) std::fprintf(stderr, "gates: ahead-of-time program %s, %u blocks\n", name, blocks);
      }
    });
    if (done) return hipGetLastError();
  }
  const GateTile tile = gates_interpreter_tile(p.n_slots, a.n_consts, env.rows);
  if (!tile.fits) return hipErrorInvalidValue;
  if (env.debug)
    std::fprintf(stderr, "gates: %zu ops, %u slots, %u constants -> %u rows per workgroup, %u waves per CU by LDS\n", p.ops.size(),
                 p.n_slots, a.n_consts, tile.rows, tile.waves);
  switch (tile.rows) {
    case 256: return launch_interpreter<256>(a, tile, stream);
    case 128: return launch_interpreter<128>(a, tile, stream);
    default: return launch_interpreter<64>(a, tile, stream);
  }
}

}  // namespace sg
