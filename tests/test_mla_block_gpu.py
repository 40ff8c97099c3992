"""The multi-head latent attention block of llama.cpp-omni_amd/mla.py on the GPU at the model's head sizes and toy width (-m gpu): kv_lora_rank 512, rope
part 64, nope part 128, V head 128, 8 heads, n_embd 256, F16 weights -- after the absorption one KV head with K rows 576 and V rows 512 wide, in separate
F16 caches.  One graph stores 33 prompt tokens into the empty caches and attends to them, then three one-token graphs run against the growing caches; the
reference CPU backend runs the same graphs on the same weights.

Bar: the FLASH_ATTN_EXT node (marked as an output) within NMSE 5e-4 per row, the block output within 5e-4 over the whole output and per token.  The same
graphs run again with option "fattn_wide" = 0 -- the generic kernel, the path before k_fattn_wide existed -- and are held to the same bar: the chain behind the
attention (wv_b, wo) does not need a wider one.  Each graph must launch k_fattn_wide at least once ("fattn_wide_launches")."""
import numpy as np
import pytest

import fattn_needle as fn
from conftest import nmse

pytestmark = pytest.mark.gpu

BAR = 5e-4
N_CTX, N_KV = 64, 64


def _run(blk, be, nt, pos0, xv):
    g, I, N = blk.build(nt, N_KV)
    N["fattn"].t.flags |= 2                                            # GGML_TENSOR_FLAG_OUTPUT
    blk.set_inputs(I, xv, pos0, N_KV)
    be.graph_compute(g.graph())
    H, R = blk.hp["n_head"], blk.hp["kv_lora_rank"]
    rows = be.tensor_get(N["fattn"]).astype(np.float64).reshape(1, nt, H, R)
    out = be.tensor_get(N["out"]).astype(np.float64).reshape(1, nt, 1, blk.hp["n_embd"])
    g.free()
    return rows, out


def test_mla_block_prompt_then_decode(pkg, be, ref_be):
    from llama_cpp_omni_amd import mla
    hp = mla.TINY_MLA
    ref = mla.MLABlock(ref_be, hp, n_ctx=N_CTX, seed=4)
    gpu = mla.MLABlock(be, hp, n_ctx=N_CTX, seed=4, weights=ref.weights)
    rng = np.random.default_rng(12)
    pos0 = 0
    try:
        for nt in (33, 1, 1, 1):
            xv = rng.standard_normal((nt, hp["n_embd"])).astype(np.float32)
            rows_ref, out_ref = _run(ref, ref_be, nt, pos0, xv)
            for wide in (-1, 0):
                be.set_option("fattn_wide", wide)
                try:
                    n0 = be.get_stat("fattn_wide_launches")
                    rows, out = _run(gpu, be, nt, pos0, xv)
                    launched = int(be.get_stat("fattn_wide_launches") - n0)
                finally:
                    be.set_option("fattn_wide", -1)
                assert np.isfinite(rows).all() and np.isfinite(out).all()
                e_row, at, _ = fn.check_rows(rows, rows_ref)
                e_tok, at_o, _ = fn.check_rows(out, out_ref)
                e_out = nmse(out, out_ref)
                print(f"mla block, {nt} tokens at {pos0}, fattn_wide {wide}: attention worst row {e_row:.3e} at {at}, block output {e_out:.3e}, worst token {e_tok:.3e}; "
                      f"k_fattn_wide launches {launched}")
                assert e_row < BAR, (nt, pos0, wide, e_row, at)
                assert e_out < BAR and e_tok < BAR, (nt, pos0, wide, e_out, e_tok, at_o)
                assert (launched >= 1) if wide else launched == 0, (nt, wide, launched)
            pos0 += nt
        kc_ref = ref_be.tensor_get(ref.k_cache).astype(np.float64)
        kc = be.tensor_get(gpu.k_cache).astype(np.float64)
        assert nmse(kc, kc_ref) < 1e-5                                  # the rows the four graphs stored (f16 roundings of f32 values that differ in the last bits)
    finally:
        ref.wctx.free()
        gpu.wctx.free()
