/* summa_verifier.h -- C ABI of the batch verifier for the constraint system of the reference's MstInclusionCircuit, exported by
 * the same shared library as include/summa_gpu.h and include/summa_prover.h.
 *
 * sp_verify_proof (summa_prover.h) checks one proof: one 37-point MSM on the device, one host wait, one two-pairing check
 * (1.3 ms of host CPU).  The reference's workload is thousands of inclusion proofs per snapshot under ONE verifying key, and
 * halo2 ships a `BatchVerifier` for exactly that.  Every commitment enters a proof's final check linearly, so N proofs fold into
 * one check with random multipliers r_i:
 *     e( sum_i r_i L_i, [1]_2 ) * e( sum_i r_i (-W'_i), [s]_2 ) == 1
 * The group side is one launch of 2 N small MSMs kept on the device (sg_msm_g1_many_begin) and sums over ranges of them
 * (sg_msm_g1_many_sums): a batch with no bad proof costs ONE pairing check; a rejected batch is bisected down to the bad proofs
 * over the same device-resident sums, with about 2 log2 N pairing checks per bad proof and nothing recomputed.
 *
 * Conventions as in summa_gpu.h: 0 or a negative sg_status; sv_last_error() (thread-local) explains a failure. */
#ifndef SUMMA_VERIFIER_H
#define SUMMA_VERIFIER_H

#include <stddef.h>
#include <stdint.h>

#include "summa_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_proofs proofs under one verifying key (passed as data, as to sp_verify_proof: k, N_CURRENCIES, the digest, the fixed and
 * permutation commitments, g2 and s_g2).  proofs[i] / proof_lens[i]: the proof's bytes; instances[i] / n_instances[i]: its instance
 * column, n x 32 B Montgomery Fr; transcript: 0 = Keccak (EVM), 1 = Blake2b, as SP_TRANSCRIPT_* of summa_prover.h.
 * entropy: 32 bytes of the caller's randomness, or NULL.  The multipliers are derived by Keccak from the key's digest, every
 * proof and instance of the batch and the entropy, so a prover who does not know the whole batch cannot aim at them; a caller
 * who verifies proofs an adversary chose TOGETHER should pass entropy.
 * accepted[i] (0 / 1) is what sp_verify_proof answers for proof i alone, always: a proof that cannot be checked (wrong length, a
 * point off the curve, an unreduced scalar or instance) is a rejection, not an error.  *pairings (may be NULL) receives the
 * number of pairing checks made: 1 for a batch with no bad proof (0 if no proof survived the host part).
 * n_proofs == 0: SG_OK, nothing written.  n_proofs > 8192, a null pointer, an unknown transcript: SG_ERR_INVALID.  The per-proof
 * host part (transcript replay, SHPLONK's scalars) runs on the calling thread. */
int sv_verify_batch(uint32_t k, uint32_t n_currencies, const uint8_t vk_digest_be[32], const uint8_t* fixed_comms,
                    const uint8_t* permutation_comms, const uint8_t g2[128], const uint8_t s_g2[128],
                    const uint8_t* const* proofs, const size_t* proof_lens, const uint8_t* const* instances,
                    const uint32_t* n_instances, uint32_t n_proofs, int transcript, const uint8_t entropy[32],
                    uint8_t* accepted, uint32_t* pairings);
const char* sv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
