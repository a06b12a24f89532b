"""The shape of the reference's criterion bench (zk_prover/benches/full_solvency_flow.rs: LEVELS = 20, k = 13), its six
entries on the device: build the Merkle sum tree of 2^LEVELS synthetic users (:18-33), build it sorted by username (:35-50),
generate the verifying key (:52-68: the 17 commitments) and the proving key (:70-86: the coefficient / coset forms), generate
the proof (:88-116: `full_prover`, Blake2b transcript) and verify it (:118-150: `full_verifier`); plus the inclusion witness of
one user in the reference circuit's own floor plan (mst_inclusion.reference_assignment) and the Keccak-flavour create_proof.
`build(levels, k)` returns everything a caller needs (tests/test_gpu_prover.py verifies the proof); run as a script
it prints the timings.  With `--csv PATH` the snapshot is a real one: the tree is DeviceMerkleSumTree.from_csv of that file
(its depth is LEVELS, its header gives the currencies) and the proof is the first user's."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch
import circuits_halo2_amd as sg
from circuits_halo2_amd import ffi, prover, arithmetic as A, mst_inclusion as M
from circuits_halo2_amd.utils import ints_to_fr, random_fr_canonical

R = M.R


def build(levels=20, k=13, user=123457, nc=2, timings=None):
    t = {} if timings is None else timings
    size = 1 << levels
    d_users = A.fr_random(bytes(range(32)), 1, size)                       # usernames: any field elements
    bal = random_fr_canonical(77, size * nc).reshape(-1, 32).copy()
    bal[:, 5:] = 0                                                         # 40-bit balances: sums stay below 2^64 (N_BYTES = 8)
    d_bals = A.fr_to_montgomery(torch.from_numpy(bal.reshape(-1)).cuda())
    nodes = 2 * size - 1
    d_h = torch.empty(32 * nodes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(32 * nodes * nc, dtype=torch.uint8, device="cuda")
    run_build = lambda: ffi.check(ffi.lib().sg_mst_build_dev(ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals), C.c_uint32(levels), C.c_uint32(nc),
                                                             ffi.dev_ptr(d_h), ffi.dev_ptr(d_b), ffi.current_stream_ptr()))
    run_build(); torch.cuda.synchronize()
    t0 = time.perf_counter(); run_build(); torch.cuda.synchronize()
    t["mst_build_ms"] = (time.perf_counter() - t0) * 1e3
    # `from_csv_sorted` [REF merkle_sum_tree/mst.rs: entries sorted by username before the tree is built]: order the 256-bit
    # usernames on the device (four stable 64-bit sorts, least significant limb first), gather the entries, build
    def run_sorted():
        canon = A.fr_from_montgomery(d_users).view(torch.int64).reshape(size, 4)
        order = torch.arange(size, device="cuda")
        for limb in range(4):
            key = canon[order, limb] ^ (-(1 << 63))                    # unsigned order on signed 64-bit keys
            order = order[torch.sort(key, stable=True).indices]
        su = d_users.view(size, 32)[order].reshape(-1)
        sb = d_bals.view(size, 32 * nc)[order].reshape(-1)
        ffi.check(ffi.lib().sg_mst_build_dev(ffi.dev_ptr(su), ffi.dev_ptr(sb), C.c_uint32(levels), C.c_uint32(nc),
                                             ffi.dev_ptr(d_hs), ffi.dev_ptr(d_bs), ffi.current_stream_ptr()))
        return su
    d_hs, d_bs = torch.empty_like(d_h), torch.empty_like(d_b)
    run_sorted(); torch.cuda.synchronize()
    t0 = time.perf_counter(); su = run_sorted(); torch.cuda.synchronize()
    t["mst_build_sorted_ms"] = (time.perf_counter() - t0) * 1e3
    if size <= (1 << 20):   # the order is the integers' order, and the root's balances do not depend on it
        first = A.fr_from_montgomery(su[:32 * 4096]).cpu().numpy().reshape(-1, 32)
        as_int = [int.from_bytes(bytes(r), "little") for r in first]
        assert as_int == sorted(as_int)
        assert (d_bs[-32 * nc:] == d_b[-32 * nc:]).all()
    # the user's path: sibling (hash, balances) per level, bottom-up (level-major node arrays)
    t0 = time.perf_counter()
    rinv = pow(1 << 256, -1, R)
    toi = lambda tens: [int.from_bytes(bytes(row), "little") * rinv % R for row in tens.cpu().numpy().reshape(-1, 32)]
    offs = [0]
    for level in range(levels):
        offs.append(offs[-1] + (size >> level))
    node_h = lambda level, i: toi(d_h[32 * (offs[level] + i):32 * (offs[level] + i) + 32])[0]
    node_b = lambda level, i: toi(d_b[32 * (offs[level] + i) * nc:32 * (offs[level] + i + 1) * nc])
    idx, bits, pre_mid = user, [], []
    for level in range(levels):
        bits.append(idx & 1)
        s = idx ^ 1
        if level:   # the sibling middle node's preimage: its balances, its children's hashes
            pre_mid.append(node_b(level, s) + [node_h(level - 1, 2 * s), node_h(level - 1, 2 * s + 1)])
        idx >>= 1
    sib = user ^ 1
    pre_leaf = toi(d_users[32 * sib:32 * sib + 32]) + toi(d_bals[32 * sib * nc:32 * (sib + 1) * nc])
    username = toi(d_users[32 * user:32 * user + 32])[0]
    balances = toi(d_bals[32 * user * nc:32 * (user + 1) * nc])
    root = (node_h(levels, 0), node_b(levels, 0))
    leaf = node_h(0, user)
    # the reference circuit's own floor plan (mst_inclusion.reference_assignment), as its keygen / prover would lay it out
    asg = M.reference_assignment(k, username, balances, bits, pre_leaf, pre_mid)
    t["witness_assignment_host_ms"] = (time.perf_counter() - t0) * 1e3
    assert asg["instances"] == [leaf, root[0]] + root[1], "the assignment's public inputs are the device tree's leaf / root"
    return asg


def build_from_csv(path, k=13, nc=2, user=0, timings=None):
    """`build` for a snapshot given as the reference's CSV (`username,balance_<name>_<chain>,...`): the entries become field
    elements on the device and the tree stays there (DeviceMerkleSumTree.from_csv); -> (assignment, levels)"""
    from circuits_halo2_amd import api
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    t = {} if timings is None else timings
    DeviceMerkleSumTree.from_csv(path, nc)
    t0 = time.perf_counter(); tree = DeviceMerkleSumTree.from_csv(path, nc)       # synchronized when it returns
    t["mst_from_csv_ms"] = (time.perf_counter() - t0) * 1e3
    t["csv_ingest"] = tree.csv_ingest                         # "device", or "host" for a file outside the device reader's subset
    t0 = time.perf_counter()
    asg = api.MstInclusionCircuit.init(tree.generate_proof(user), tree.depth, nc).synthesize(k)
    t["witness_assignment_host_ms"] = (time.perf_counter() - t0) * 1e3
    assert asg["instances"] == tree.public_inputs(user), "the assignment's public inputs are the device tree's leaf / root"
    return asg, tree.depth


def keygen_and_prove(asg, k, params, reps=3, timings=None, nc=2):
    t = {} if timings is None else timings
    dev = lambda v: torch.from_numpy(ints_to_fr(v)).cuda()
    fixed, sigma, advice = [dev(c) for c in asg["fixed"]], [dev(c) for c in asg["sigma"]], [dev(c) for c in asg["advice"]]
    pk = prover.ProvingKey(params, k, fixed, sigma, nc)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    pk = prover.ProvingKey(params, k, fixed, sigma, nc)
    t["keygen_ms"] = (time.perf_counter() - t0) * 1e3
    # the two halves as the reference benches them: keygen_vk = the 17 commitments, keygen_pk = the transforms
    torch.cuda.synchronize(); t0 = time.perf_counter()
    params.commit_batch(fixed + sigma, lagrange=True)
    t["keygen_vk_ms"] = (time.perf_counter() - t0) * 1e3
    t["keygen_pk_ms"] = max(0.0, t["keygen_ms"] - t["keygen_vk_ms"])
    proof = prover.create_proof(params, pk, advice, asg["instances"])
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        proof = prover.create_proof(params, pk, advice, asg["instances"])
        best = min(best, (time.perf_counter() - t0) * 1e3)
    t["create_proof_ms"] = best
    # full_prover / full_verifier: the Blake2b flavour, the product's verifier (GPU MSM + host pairing)
    from circuits_halo2_amd import api, verifier
    vk = api.VerifyingKey(k, nc, pk.fixed_comms, pk.permutation_comms, pk.vk_digest)
    best_p, best_v = 1e9, 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        blake = prover.create_proof(params, pk, advice, asg["instances"], transcript=prover.Blake2bWrite())
        best_p = min(best_p, (time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ok = verifier.verify_proof(params, vk, blake, asg["instances"], flavour="blake2b")
        best_v = min(best_v, (time.perf_counter() - t0) * 1e3)
        assert ok
    t["full_prover_ms"], t["full_verifier_ms"], t["verified"] = best_p, best_v, True
    return pk, advice, proof


def run(levels=20, k=13, cpp=True, nc=2, csv=None):
    import json, subprocess, tempfile
    t = {}
    if csv is not None:
        asg, levels = build_from_csv(csv, k, nc=nc, timings=t)
    else:
        asg = build(levels, k, nc=nc, timings=t)
    params = sg.ParamsKZG.setup(k, ints_to_fr([0x1D0C0FFEE1234567890ABCDEF]))
    params.precompute()
    pk, advice, proof = keygen_and_prove(asg, k, params, timings=t, nc=nc)
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "create_proof_cpp")
    if cpp and os.path.exists(exe):
        with tempfile.TemporaryDirectory() as td:
            prover.export_bundle(os.path.join(td, "b.bin"), params, pk, advice, asg["instances"])
            r = subprocess.run([exe, os.path.join(td, "b.bin"), os.path.join(td, "p.bin"), "8"], capture_output=True, text=True, timeout=300)
            if r.returncode == 0:
                t["create_proof_ms_cpp_driver"] = json.loads(r.stdout.strip().splitlines()[-1])["create_proof_ms"]
    params.free()
    t.update({"levels": levels, "k": k, "n_currencies": nc, "rows_used": asg["rows_used"]})
    return t


if __name__ == "__main__":
    ffi.check(ffi.lib().sg_init(0))
    argv, csv_path = sys.argv[1:], None
    if "--csv" in argv:                       # [LEVELS [K [N_CURRENCIES]]] --csv PATH: LEVELS is then the tree's own depth
        at = argv.index("--csv")
        csv_path = argv[at + 1]
        del argv[at:at + 2]
    print(run(int(argv[0]) if len(argv) > 0 else 20, int(argv[1]) if len(argv) > 1 else 13,
              nc=int(argv[2]) if len(argv) > 2 else 2, csv=csv_path))
