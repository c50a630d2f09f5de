"""The attention forms of the dispatch and the ragged lengths, shared by tests/test_gpu_ragged.py, tests/planted_attention.py and the
tests built on it (a table only: importing it needs no GPU)."""
from egoego_release_amd import _lib

P3, P8, P9 = _lib.PREC_BF16X3, _lib.PREC_I8X3, _lib.PREC_I8X3_FC
S6, S3, S2, AW, CS = "attn_proj6_i8_kernel", "attn_proj_i8_kernel", "attn_proj2_i8_kernel", "attn_layer_i8w_kernel", "attn_core_s_kernel"
# the padded length first (every batch also holds an unpadded window), then the key-tile edges
LENGTHS = {120: (120, 11, 31, 32, 63, 64, 95, 96, 119), 196: (196, 11, 31, 32, 127, 128, 159, 160, 191, 192, 195), 30: (30, 1, 11, 29),
           40: (40, 11, 25, 33, 12)}
# (precision, T, B) -> (qkv, attn) kernels, names as in tests/test_gpu_dispatch.py
FORMS = [
    (P3, 120, 2, "qkv_kernel", "attn_kernel"),
    (P3, 120, 48, "qkv_attn_kernel", "qkv_attn_kernel"),
    (P3, 196, 2, "qkv_kernel", "attn_kernel"),  # KT 7
    (P3, 196, 64, "qkv_kernel", "attn8_kernel"),
    (P3, 30, 3, "qkv_kernel", "attn_kernel"),  # KT 1
    (P8, 120, 2, S6, CS), (P9, 120, 2, S6, CS),
    (P8, 120, 11, S3, CS), (P9, 120, 11, S3, CS),
    (P8, 120, 22, S2, CS), (P9, 120, 22, S2, CS),
    (P8, 120, 25, AW, AW), (P9, 120, 25, AW, AW),
    (P8, 196, 2, "qkv_i8q_kernel", "attn_core_i8w_kernel"), (P9, 196, 2, "qkv_i8q_kernel", "attn_core_i8w_kernel"),
    (P8, 30, 3, "qkv_i8_kernel", "attn_kernel"),
]


def lens(T, B, shift=0):
    c = LENGTHS[T]
    return [c[(b + shift) % len(c)] if b else c[0] for b in range(B)]
