"""Flag values of include/ecsimd_hip.h (scalar_mult `flags`)."""
BASE_CLASSICAL = 0
BASE_MGRY = 1
OUT_JACOBIAN = 0
OUT_AFFINE = 2
ALG_WINDOWED = 4
ALG_WINDOWED_SIGNED = 8
ALG_NO_ENDOMORPHISM = 16
ALG_WINDOWED_BIG = 32
REF_SQUARE_COMPAT = 64
ALG_CONSTANT_TIME = 128       # scalar_mult_base + ALG_WINDOWED: every table entry read, the wanted one kept under lane masks
BASE_GENERATOR = 512          # ecsimd_hip_scalar_mult with x = y = NULL: the base point is the generator
LADDER_RADIX32 = 256          # ladder only: the loop on 8 x 32-bit canonical words (rounds 1-3) instead of nine signed 29-bit limbs
GROUP_NO_GATHER = 0x10000    # ecsimd_hip_group_scalar_mult only: compute without the exchange
ECDSA_LOW_S = 1               # ecsimd_hip_ecdsa_sign_recoverable only: s > n / 2 is returned as n - s (and bit 0 of v flipped)
ETH_REQUIRE_LOW_S = 1         # ecsimd_hip_eth_recover only: s > n / 2 is refused (EIP-2)
BIP32_ALL_HARDENED = 1        # ecsimd_hip_bip32_ckd_priv only: every index has bit 31 set (no point multiplication; a lane that breaks the promise is refused)
ED25519_REJECT_SMALL_ORDER = 1   # ecsimd_ed25519_verify only: a small-order A or R is refused as well
SCHNORR_BATCH_AUTO = 0        # ecsimd_schnorr_verify_batch only (include/ecsimd_schnorr_batch.h): LANES below ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD signatures, MSM from there on
SCHNORR_BATCH_MSM = 1         # ... the randomized sum: two bucket multi-scalar multiplications and one verdict
SCHNORR_BATCH_LANES = 2       # ... schnorr_verify's own path and one reduction
ED25519_BATCH_AUTO = 0        # ecsimd_ed25519_verify_batch / _batch_plan only (include/ecsimd_ed25519_batch.h): LANES below ECSIMD_ED25519_BATCH_AUTO_THRESHOLD signatures, MSM from there on
ED25519_BATCH_MSM = 2         # ... the randomized cofactored sum: two bucket multi-scalar multiplications on the Edwards curve and one verdict
ED25519_BATCH_LANES = 4       # ... ed25519_verify_cofactored's own path and one reduction; all three or-able with ED25519_REJECT_SMALL_ORDER
