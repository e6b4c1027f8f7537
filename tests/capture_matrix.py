"""Every function of include/ecsimd_hip.h in exactly one class of behaviour under hipGraph stream capture.

Classified by reading each entry point's host path in ecsimd_amd/csrc/capi.hip and group.hip -- not by trying it on a GPU.  Names are the ABI's without the
`ecsimd_hip_` prefix.  tests/test_capture_matrix_cpu.py holds this file to the header (a declared function in no class, in two, or a listed name that is no
longer declared fails it) and tests/test_gpu_graph_capture.py to this file (one case per CAPTURABLE and per REFUSES name).  A new entry point is classified
here by whoever adds it.

CAPTURABLE  once warmed up (the first call at the capture's batch size has sized the context workspace and built the tables the call needs) the host path does
            nothing but enqueue on the context's stream: kernel launches, hipMemsetAsync wipes of the workspace, device-to-device copies.  Host scalars and
            host arrays of a fixed few words (mgry_pow's exponent, scalar_mult_1s's k1) are kernel arguments: taken by value when the call is captured.
REFUSES     needs the host: hands a value back, copies from or to memory that may be pageable, waits for the stream, allocates or frees, times with events.
            Under capture: ECSIMD_HIP_ERR_BAD_ARG with "capture" in ecsimd_hip_last_error, checked BEFORE the stream is touched -- nothing enqueued, the
            capture stays valid.
NO_STREAM   no part of a stream's work: enqueues nothing on the context's stream and waits for nothing on it (or has no context at all) -- with ONE exception,
            destroy, which waits for the stream once, to end the context, and so must not be called while that stream is being captured.  One line of reason each.
"""

CAPTURABLE = [
    # stream selection: an event hand-off outside a capture, the bare handle under one (capi.hip switch_stream)
    "set_stream", "use_own_stream",
    "memcpy_d2d",
    # L2
    "add", "sub", "sub_if_above", "cmp_eq", "mask_op", "cmp_lt", "shift_left_one", "mul", "square", "swap_if", "if_else",
    # wire formats
    "from_bytes_be", "to_bytes_be", "wide4_to_lanes", "lanes_to_wide4", "mask_bit", "sec1_encode", "sec1_decode",
    # L3
    "mod_add", "mod_sub", "mod_shift_left", "mod_mul", "mgry_reduce", "mgry_mul", "mgry_sqr", "mgry_from_classical", "mgry_to_classical", "mgry_pow",
    "gfp_inverse", "gfp_opposite", "gfp_sqrt",
    # L4 / L5
    "from_affine", "to_affine", "compute_y", "dblu", "zaddu", "zdau", "zdau_repeat", "add_z2_1", "add_mixed_complete", "trplu",
    "scalar_mult", "scalar_mult_1s", "scalar_mult_base", "scalar_mult_p256", "affine_add", "on_curve", "double_scalar_mult",
    # ECDSA
    "ecdsa_verify_rx", "ecdsa_verify", "ecdsa_sign", "ecdsa_recover", "ecdsa_sign_recoverable", "sha256", "rfc6979_nonce", "ecdsa_sign_deterministic",
    # BIP-340
    "schnorr_verify", "schnorr_sign",
    # Ethereum
    "keccak256", "eth_address", "eth_recover",
    # Bitcoin
    "ripemd160", "hash160", "sha256d", "sha256_lens", "sha256d_lens", "hash160_lens", "ripemd160_lens", "tapleaf_hash", "taproot_merkle_path", "btc_pubkey_hash",
    "xonly_tweak_add", "taproot_tweak_pubkey", "taproot_tweak_seckey",
    # BIP-32 / BIP-39
    "sha512", "hmac_sha512", "bip32_master", "bip32_ckd_priv", "bip32_ckd_pub", "pbkdf2_hmac_sha512", "bip39_seed",
    # diagnostics and synthetic inputs
    "fe29_raw", "fill_random",
]

REFUSES = {
    "sync": "hipStreamSynchronize on the context's stream",
    "malloc": "hipMalloc: an allocation is not a stream operation and is not allowed while a capture is open",
    "free": "hipFree waits for the device",
    "memcpy_h2d": "copies from host memory that may be pageable, then waits for the stream",
    "memcpy_d2h": "copies to host memory, then waits for the stream",
    "mask_count": "returns the count to the host: a copy into a stack variable and a wait",
    "scalar_mult_host": "host arrays in and out: staging allocations, copies and waits on two streams",
    "btc_merkle_root": "reads tree_offsets on the host and uploads the node offsets from a pinned block it may have to allocate and wait for",
    "peak_mad32": "creates two events, times its launches with them and waits for the second",
}

NO_STREAM = {
    "init": "creates the context and its own stream; there is no stream to capture yet",
    "destroy": "ends the context's life: WAITS for its stream, then frees what it owns -- must not be called while that stream is captured (it would invalidate the capture)",
    "set_ref_square_compat": "sets a field of the context on the host",
    "get_ref_square_compat": "reads a field of the context on the host",
    "last_error": "returns the context's message buffer",
    "version": "returns a string literal",
    "get_constant": "host arithmetic on the curve's constants; takes no context",
    "register_modulus": "process-wide registry on the host; takes no context",
    "register_curve": "process-wide registry on the host; takes no context",
    "curve_capabilities": "reads the registry on the host; takes no context",
    "workspace_info": "returns the workspace's pointer and size from the context, touches neither",
    "shard_range": "pure host arithmetic",
    "group_init": "creates a group's own contexts and streams",
    "group_destroy": "destroys a group's own contexts and streams",
    "group_size": "reads a field of the group",
    "group_uses_rccl": "reads a field of the group",
    "group_rccl_version": "reads a field of the group",
    "group_context": "returns a member's context pointer",
    "group_last_error": "returns the group's message buffer",
    "group_scalar_mult": "runs on the streams of the group's own member contexts, which no caller hands to a capture",
    "group_sync": "waits for the group's own streams",
    "group_member_ms": "reads the events of a member's own stream",
    "group_rccl_selftest": "allocates, copies and waits on the group's own gather stream",
    "group_scalar_mult_host": "synchronous host-array form over the group's own streams",
}

CLASSES = {"CAPTURABLE": CAPTURABLE, "REFUSES": REFUSES, "NO_STREAM": NO_STREAM}
