// What the translation units of the C ABI share (summa_gpu.hip: the core; abi_msm / abi_ntt / abi_poly / abi_quotient / abi_mst.hip:
// the entry points by family).  Private to csrc/: the public interface is include/summa_gpu.h alone.
#pragma once
#include "../../include/summa_gpu.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "host_curve.h"
#include "host_pairing.h"
#include "../../include/summa_prover.hpp"
#include "../../include/summa_circuit.hpp"
#include "msm.h"
#include "ntt.h"
#include "quotient.h"
#include "gates.h"
#include "numerator.h"
#include "poly.h"
#include "witness.h"
#include "side_prio.cuh"
#include "host_wait.h"

namespace sg {

extern thread_local char g_err[512];   // sg_last_error's text
int fail(int code, const char* what, hipError_t e = hipSuccess);
int hip_fail(const char* what, hipError_t e);
#define CHECK_HIP(call, what)                  \
  do {                                         \
    hipError_t _e = (call);                    \
    if (_e != hipSuccess) return hip_fail(what, _e); \
  } while (0)

// BN254 Fr constants as Montgomery-2^256 words (one copy per translation unit: no relocatable device code)
static __device__ const uint32_t ROOT_OF_UNITY_M[8] = {0xb639feb8u, 0x9632c7c5u, 0x0d0ff299u, 0x985ce340u,
                                                       0x01b0ecd8u, 0xb2dd8800u, 0x6d98ce29u, 0x1d69070du};  // order 2^28
static __device__ const uint32_t ZETA_M[8] = {0x55fcd653u, 0x0363f299u, 0x5fc1e200u, 0x73e7950bu,
                                              0x576d9d24u, 0xc5fce83eu, 0xa1c3a4d4u, 0x059c805du};  // Fr::ZETA
// delta = 7^(2^28): generator of the 2^28-torsion-free part used to separate permutation columns
static const words8 DELTA_M = {{0xefd78855u, 0x9a0c322bu, 0x249b563cu, 0x46e82d14u,
                                 0xe0b0b7a7u, 0x5983a663u, 0xaaa111adu, 0x22ab452bu}};  // Montgomery-2^256 words

struct DomainConsts {  // all Montgomery-2^256 words
  words8 omega, omega_inv, n_inv, zeta, zeta2, ninv_zeta2, ninv_zeta, one;
};

struct Srs {
  uint32_t k;
  g1_affine_mem* g;
  g1_affine_mem* g_lagrange;
  FixedTable tab[3];  // optional precomputed window tables (sg_srs_precompute): [0] g, [1] g_lagrange, [2] the prefix sums
                      // of g_lagrange (difference-form commitments of Lagrange columns)
  g1_affine_mem* lagrange_prefix = nullptr;   // made with tab[2]
};

struct ManyJobs {   // behind a handle of sg_msm_g1_many_begin: the window sums of `jobs` small MSMs, on the device
  uint32_t jobs;
  uint32_t* S;
};

struct Context {
  int device = -1;
  hipStream_t stream = nullptr;
  NttEngine ntt;
  MsmEngine msm, msm_b;          // two engines: batches ping-pong between them
  WitnessEngine witness;
  hipStream_t bstream[2] = {nullptr, nullptr};
  hipStream_t tstream[2] = {nullptr, nullptr};  // high-priority tails
  hipEvent_t ev_in = nullptr;
  DevBuf<uint8_t> stage_a, stage_b, scratch;
  std::vector<uint8_t> gate_blob_host;
  GateProgramCache gate_programs;   // lowered gate programs by structure (gates_compile.h)
  // work space of the scan-type helpers (prefix / grand products, Kate division) and the scratch vector of in-place multi-pass
  // transforms: per (stream, slot), so that the calls are asynchronous -- work on one stream is ordered, other streams own
  // other buffers
  std::map<std::pair<hipStream_t, int>, DevBuf<uint8_t>> stream_scratch;
  DomainConsts* d_consts = nullptr;
  struct CosetTables {       // sg_coeff_to_cosets / sg_cosets_to_pieces: per (k, ext_k, cosets)
    fp_words* fwd = nullptr;  // [nc][n] c_b^i   (2^261-domain words)
    fp_words* inv = nullptr;  // [nc][n] c_b^-i
    words8 shift[MAX_COSETS]; // c_b = zeta omega_ext^b
    uint32_t m[MAX_COSETS * MAX_COSETS][8];   // V^-1 diag(1 / (c_b^n - 1)), row-major [t][b]
  };
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, CosetTables> coset_tables;
  struct BlobSlot {   // a page-locked host / device buffer pair in flight; ev: recorded behind the work that reads it
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
  };
  struct BlobRing {   // (ring_slot, below)
    uint32_t size;   // slots in use: at most the 16 of `slot` (the others stay empty)
    uint32_t next = 0;
    BlobSlot slot[16];
  };
  BlobRing blob_ring{16};   // sg_quotient_gates: program blobs
  // sg_fr_kate_division_batch: the divisions' power tables (host-computed, 684 B each) on their way to the device, so that the call
  // returns without waiting for the stream
  BlobRing kate_ring{4};
  std::map<uint32_t, DomainConsts> consts;
  std::map<uint64_t, fp_words*> t_evals;  // key = k << 32 | ext_k
  // page-locked host memory mapped into the device: small results the host waits for anyway (evaluations, a remainder, a
  // verdict) are written there by the kernel that produces them -- no copy kernel, no second wait
  static constexpr size_t MAIL_BYTES = 4096;
  uint8_t* h_mail = nullptr;
  uint8_t* d_mail = nullptr;
  // sg_msm_g1_many_sums: the window sums of up to MSM_MANY_MAX_RANGES ranges, mapped the same way (64 KB)
  uint32_t* h_many = nullptr;
  uint32_t* d_many = nullptr;
  // sg_lookup_permute_small_async_dev: two work spaces per caller stream; the write pass of one call zeroes the other's
  // histograms for the next call (no memset launches)
  struct LookupWork {
    DevBuf<uint32_t> buf;
    uint32_t next = 0;
  };
  std::map<hipStream_t, LookupWork> lookup_work;
};

// the rows of kParams (summa_gpu.hip, defined beside it) the families read in Shared::param
extern const size_t kRowCombineWaitUs, kRowCombineTarget, kRowCombineRunners, kRowHostChunks, kRowTinyMax, kRowCosetScalePass,
    kRowFusedNumerator, kRowFailNextFusedJob;
constexpr size_t kMaxParams = 64;   // kParams fits (asserted beside it)

// What every lane shares: the device index, the SRS cache (read-only after upload / precompute) and the runtime
// parameters.  Guarded by its own short mutex (never held across device work).
struct Shared {
  std::mutex mu;
  int device = -1;
  std::map<uint64_t, Srs> srs;
  std::map<uint64_t, ManyJobs> many;   // live handles of sg_msm_g1_many_begin
  uint64_t next_handle = 1;
  std::atomic<int> param[kMaxParams];   // the value in effect of each row of kParams: written under mu, read anywhere
  Shared();
};
extern Shared g_sh;
extern thread_local Context* g_ctx;   // the lane this thread holds (valid inside LOCKED_CTX scopes only)
extern thread_local int g_depth;      // how many LaneHolds of this thread are open (the lane lock is re-entrant)
struct LaneHold {
  int rc = SG_OK;
  LaneHold();
  ~LaneHold();
  LaneHold(const LaneHold&) = delete;
  LaneHold& operator=(const LaneHold&) = delete;
};

inline words8 load32(const uint8_t* p) {   // a 32-byte argument (a field element as Montgomery words)
  words8 w;
  std::memcpy(&w, p, 32);
  return w;
}
void msm_set(Context& c, uint32_t MsmConfig::*field, int v);
bool find_srs(uint64_t handle, Srs* out);
int get_consts(uint32_t k, const DomainConsts** out);
hipStream_t pick_stream(void* s);
int sync_own_stream_into(hipStream_t s);
int ntt_dev(const fp_words* in, size_t in_len, fp_words* out, uint32_t log_n, const words8& omega,
            const words8* scale, const words8* pre3, const words8* post3, hipStream_t s);
hipError_t mailbox(uint8_t** host, uint8_t** dev);
hipError_t scratch_for(hipStream_t s, int slot, size_t bytes, uint8_t** out);
// The next slot of a ring of page-locked host / device buffer pairs, with room for `bytes` (a smaller one is replaced by one of
// `grow_to` bytes) and free: the work that read it last has run (an event; normally long complete, so no host wait unless the
// ring has wrapped onto a launch that is still running).  The caller records (*out)->ev behind the work that reads the slot.
hipError_t ring_slot(Context::BlobRing& ring, size_t bytes, size_t grow_to, Context::BlobSlot** out);
int upload(DevBuf<uint8_t>& buf, const uint8_t* host, size_t bytes, hipStream_t s);
int download(uint8_t* host, const void* dev, size_t bytes, hipStream_t s);
// abi_ntt.hip
int coset_tables_for(uint32_t k, uint32_t ext_k, uint32_t nc, const Context::CosetTables** out);
bool coset_shape_ok(uint32_t k, uint32_t ext_k, uint32_t nc);
// t_eval_kernel (abi_ntt.hip's table of 1 / (X^n - 1)) and kzg_setup_scalars (abi_poly.hip) on `s`: summa_gpu.hip holds the kernels
void t_eval_launch(uint32_t k, uint32_t ext_k, const words8& omega_ext, fp_words* out, hipStream_t s);
void kzg_setup_scalars_launch(uint32_t k, const words8& tau, fp_words* pw, fp_words* lg, hipStream_t s);

#define LOCKED_CTX()     \
  LaneHold _hold;        \
  if (_hold.rc != SG_OK) return _hold.rc;
#define TRY(x)                  \
  do {                          \
    int _rc = (x);              \
    if (_rc != SG_OK) return _rc; \
  } while (0)

}  // namespace sg
