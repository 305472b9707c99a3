"""Torch-tensor front end of the primitive C-ABI operators (include/vitron_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function below checks its tensors,
passes raw device pointers + the current stream to libvitron_hip.so and returns torch tensors. There is no
torch-op fallback: without the shared library, or on a CPU tensor, these raise.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (CFG_AUTO, EPI_BF16, EPI_BF16_GELU, EPI_BF16_QGELU, EPI_BF16_RELU, EPI_F32, EPI_F32_RESID,  # noqa: F401
                   EPI_SWIGLU_BF16, PAGE_TOKENS)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _op16(t: torch.Tensor, name: str):
    """(library, dtype) for a 16-bit operand tensor: its dtype (bf16 / fp16) picks the library build."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitronHipError(f"{name}: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.VitronHipError(f"{name}: expected a bf16 or fp16 tensor, got {t.dtype}")
    return _lib.lib_for(t), t.dtype


def _chk(t: torch.Tensor, dtype, name: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitronHipError(f"{name}: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if t.dtype != dtype:
        raise _lib.VitronHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.VitronHipError(f"{name}: tensor must be contiguous")


def _chk_view(t: torch.Tensor, dtype, name: str):
    """contiguous tensor, or row-strided 2-D view (stride(1) == 1, rows that do not overlap): its row stride travels as the leading dimension.
    Alignment (lda / ldw % 8, ldc % 4, 16-byte base pointers) is the C ABI's own check."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitronHipError(f"{name}: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if t.dtype != dtype:
        raise _lib.VitronHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.is_contiguous():
        return
    if t.dim() != 2 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise _lib.VitronHipError(f"{name}: expected a 2-D tensor with contiguous rows (a row-strided view at most), got shape "
                                  f"{tuple(t.shape)} strides {tuple(t.stride())}")


def gemm_plan(M: int, N: int, K: int, epi: int = EPI_BF16):
    """(cfg, rows_first) the dispatcher picks for an AUTO vt_gemm_bf16 of this shape (host logic, no launch; include/vitron_hip.h)."""
    import ctypes
    lib = _lib.load_any()
    cfg, rows = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.vt_gemm_plan_query(M, N, K, epi, ctypes.byref(cfg), ctypes.byref(rows)), "vt_gemm_plan_query", lib)
    return cfg.value, rows.value


def gemm_plan_cols(M: int, N: int, K: int, epi: int = EPI_BF16):
    """(cfg, rows_first, cols_first) of the dispatcher's plan (vt_gemm_plan_query2): cols_first > 0 = the column split of round 5."""
    import ctypes
    lib = _lib.load_any()
    cfg, rows, cols = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.vt_gemm_plan_query2(M, N, K, epi, ctypes.byref(cfg), ctypes.byref(rows), ctypes.byref(cols)), "vt_gemm_plan_query2", lib)
    return cfg.value, rows.value, cols.value


def gemm_plan_split(M: int, N: int, K: int, epi: int = EPI_BF16):
    """(cfg, rows_first, cols_first, cfg_rest) of the plan the dispatcher runs (vt_gemm_plan_query3): cols_first > 0 = columns [0, cols_first)
    on cfg -- whole rounds of 256-, 320- or 224-row tiles -- and the remaining columns on cfg_rest."""
    import ctypes
    lib = _lib.load_any()
    cfg, rows, cols, rest = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.vt_gemm_plan_query3(M, N, K, epi, ctypes.byref(cfg), ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(rest)),
               "vt_gemm_plan_query3", lib)
    return cfg.value, rows.value, cols.value, rest.value


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epi: int = EPI_BF16,
         out: Optional[torch.Tensor] = None, cfg: int = CFG_AUTO, row_scale: Optional[torch.Tensor] = None,
         colsplit: Optional[tuple] = None) -> torch.Tensor:
    """out = epi(row_scale[:, None] * (a[M,K] @ w[N,K]^T) + bias). EPI_F32_RESID accumulates into `out` (fp32, required).
    colsplit = (cols_first, cfg_rest): forced column split (vt_gemm_bf16_colsplit) -- columns [0, cols_first) on `cfg`, the rest on cfg_rest."""
    lib, dt = _op16(a, "gemm.a")
    _chk_view(a, dt, "gemm.a")
    _chk_view(w, dt, "gemm.w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VitronHipError(f"gemm: K mismatch {K} vs {K2}")
    if bias is not None:
        _chk(bias, torch.float32, "gemm.bias")
    n_out = N // 2 if epi == EPI_SWIGLU_BF16 else N
    odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else dt
    if out is None:
        if epi == EPI_F32_RESID:
            raise _lib.VitronHipError("gemm: EPI_F32_RESID needs `out` (the fp32 residual stream)")
        out = torch.empty((M, n_out), device=a.device, dtype=odt)
    _chk_view(out, odt, "gemm.out")
    if not out.is_contiguous() and tuple(out.shape) != (M, n_out):
        raise _lib.VitronHipError(f"gemm: out is a view of {tuple(out.shape)}, expected {(M, n_out)}")
    if row_scale is not None:
        _chk(row_scale, torch.float32, "gemm.row_scale")
        if row_scale.numel() != M:
            raise _lib.VitronHipError(f"gemm: row_scale has {row_scale.numel()} elements for M={M}")
    if colsplit is not None:
        if row_scale is not None:
            raise _lib.VitronHipError("gemm: a forced column split takes no row_scale")
        n1, cfg_rest = colsplit
        _lib.check(lib.vt_gemm_bf16_colsplit(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(bias), M, N, K, epi,
                                             cfg, int(n1), int(cfg_rest), _stream()), "vt_gemm_bf16_colsplit", lib)
        return out
    _lib.check(lib.vt_gemm_bf16(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(bias), M, N, K, epi,
                                cfg, _p(row_scale), _stream()), "vt_gemm_bf16", lib)
    return out


def gemm_resid_splitk(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None, ksplit: int = 0,
                      partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32) += a @ w^T + bias, optionally as a two-pass split-K through the fp32 workspace `partials`."""
    lib, dt = _op16(a, "gemm_resid_splitk.a")
    _chk_view(a, dt, "gemm_resid_splitk.a")
    _chk_view(w, dt, "gemm_resid_splitk.w")
    _chk_view(out, torch.float32, "gemm_resid_splitk.out")
    M, K = a.shape
    N = w.shape[0]
    if not out.is_contiguous() and tuple(out.shape) != (M, N):
        raise _lib.VitronHipError(f"gemm_resid_splitk: out is a view of {tuple(out.shape)}, expected {(M, N)}")
    nbytes = 0 if partials is None else partials.numel() * partials.element_size()
    _lib.check(lib.vt_gemm_bf16_resid_splitk(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(bias), M, N, K,
                                             int(ksplit), _p(partials), nbytes, _stream()), "vt_gemm_bf16_resid_splitk", lib)
    return out


def _chk_norm_out(norm_out, dt, M: int, N: int, name: str):
    """(w fp32 [N], xw op16 [M][N] -- a row-strided view at most --, partials fp32) of a folded-norm producer"""
    ow, oxw, opart = norm_out
    _chk(ow, torch.float32, name + ".norm_out.w")
    _chk_view(oxw, dt, name + ".norm_out.xw")
    _chk(opart, torch.float32, name + ".norm_out.partials")
    if ow.numel() != N or tuple(oxw.shape) != (M, N):
        raise _lib.VitronHipError(f"{name}: norm_out shapes must be w [N], xw [M][N]")
    return ow, oxw, opart


def gemm_norm(a: torch.Tensor, w: torch.Tensor, epi: int = EPI_BF16, out: Optional[torch.Tensor] = None,
              norm_in: Optional[tuple] = None, norm_out: Optional[tuple] = None) -> torch.Tensor:
    """out = epi(a[M,K] @ w[N,K]^T) on the M <= 16 weight-streaming kernel with the decode step's folded RMSNorm (include/vitron_hip.h
    vt_gemm_bf16_norm; EPI_BF16 / EPI_F32 / EPI_F32_RESID into `out` / EPI_SWIGLU_BF16), the conventions of gemm_nf4:
      norm_in  = (partials fp32 [M][in_n], inv_dim, eps): row m scaled by rsqrt(sum(partials[m]) * inv_dim + eps);
      norm_out = (w_next fp32 [N], xw op16 [M][N], partials fp32 [M][N/16]) with EPI_F32_RESID: xw = op16(x_new * w_next), partials = sums
      of x_new^2 over each 16 columns."""
    lib, dt = _op16(a, "gemm_norm.a")
    _chk_view(a, dt, "gemm_norm.a")
    _chk_view(w, dt, "gemm_norm.w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VitronHipError(f"gemm_norm: K mismatch {K} vs {K2}")
    n_out = N // 2 if epi == EPI_SWIGLU_BF16 else N
    odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else dt
    if out is None:
        if epi == EPI_F32_RESID:
            raise _lib.VitronHipError("gemm_norm: EPI_F32_RESID needs `out` (the fp32 residual stream)")
        out = torch.empty((M, n_out), device=a.device, dtype=odt)
    _chk_view(out, odt, "gemm_norm.out")
    if tuple(out.shape) != (M, n_out):
        raise _lib.VitronHipError(f"gemm_norm: out is {tuple(out.shape)}, expected {(M, n_out)}")
    pin, in_n, inv_dim, eps = None, 0, 0.0, 0.0
    if norm_in is not None:
        pin, inv_dim, eps = norm_in
        _chk(pin, torch.float32, "gemm_norm.norm_in")
        if pin.dim() != 2 or pin.shape[0] < M:
            raise _lib.VitronHipError("gemm_norm: norm_in partials must be [M][in_n]")
        in_n = pin.shape[1]
    ow = oxw = opart = None
    ld_xw = 0
    if norm_out is not None:
        ow, oxw, opart = _chk_norm_out(norm_out, dt, M, N, "gemm_norm")
        if opart.numel() < M * (N // 16):
            raise _lib.VitronHipError("gemm_norm: norm_out partials must be [M][N/16]")
        ld_xw = oxw.stride(0)
    _lib.check(lib.vt_gemm_bf16_norm(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K, epi, _p(pin), in_n,
                                     float(inv_dim), float(eps), _p(ow), _p(oxw), ld_xw, _p(opart), _stream()), "vt_gemm_bf16_norm", lib)
    return out


def gemm_resid_norm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, norm_out: tuple, bias: Optional[torch.Tensor] = None,
                    cfg: int = CFG_AUTO, ksplit: int = -1, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32) += a @ w^T + bias on the MFMA tile kernels with the folded RMSNorm's producer (include/vitron_hip.h vt_gemm_bf16_resid_norm):
    norm_out = (w_next fp32 [N], xw op16 [M][N], partials fp32 [np][ldp], np >= N/32 groups of ldp >= M rows): xw = op16(x_new * w_next),
    partials[g][m] = the sum of x_new^2 over columns [32 g, 32 g + 32). ksplit < 0: gemm's dispatcher with `cfg`; ksplit >= 0: the route of
    gemm_resid_splitk (0 = decide, >= 2 = force) through the fp32 `workspace`."""
    lib, dt = _op16(a, "gemm_resid_norm.a")
    _chk_view(a, dt, "gemm_resid_norm.a")
    _chk_view(w, dt, "gemm_resid_norm.w")
    _chk_view(out, torch.float32, "gemm_resid_norm.out")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VitronHipError(f"gemm_resid_norm: K mismatch {K} vs {K2}")
    if tuple(out.shape) != (M, N):
        raise _lib.VitronHipError(f"gemm_resid_norm: out is {tuple(out.shape)}, expected {(M, N)}")
    if bias is not None:
        _chk(bias, torch.float32, "gemm_resid_norm.bias")
    ow, oxw, opart = _chk_norm_out(norm_out, dt, M, N, "gemm_resid_norm")
    if opart.dim() != 2 or opart.shape[0] < N // 32 or opart.shape[1] < M:
        raise _lib.VitronHipError(f"gemm_resid_norm: norm_out partials must be [np >= N/32][ldp >= M], got {tuple(opart.shape)}")
    nbytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    _lib.check(lib.vt_gemm_bf16_resid_norm(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(bias), M, N, K, int(cfg),
                                           int(ksplit), _p(workspace), nbytes, _p(ow), _p(oxw), oxw.stride(0), _p(opart), opart.shape[0],
                                           opart.shape[1], _stream()), "vt_gemm_bf16_resid_norm", lib)
    return out


def rowscale_finalize(partials: torch.Tensor, rows: int, inv_dim: float, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = rsqrt(sum_g partials[g][m] * inv_dim + eps), m < rows, for partials fp32 [np][ldp >= rows]: the row_scale of the GEMM that
    consumes a gemm_resid_norm producer's xw."""
    _chk(partials, torch.float32, "rowscale_finalize.partials")
    if partials.dim() != 2 or partials.shape[1] < rows:
        raise _lib.VitronHipError(f"rowscale_finalize: partials must be [np][ldp >= rows], got {tuple(partials.shape)} for rows={rows}")
    if out is None:
        out = torch.empty((rows,), device=partials.device, dtype=torch.float32)
    _chk(out, torch.float32, "rowscale_finalize.out")
    if out.numel() < rows:
        raise _lib.VitronHipError(f"rowscale_finalize: out has {out.numel()} elements for rows={rows}")
    lib = _lib.load_any()
    _lib.check(lib.vt_rowscale_finalize(_p(partials), partials.shape[0], partials.shape[1], rows, float(inv_dim), float(eps), _p(out),
                                        _stream()), "vt_rowscale_finalize", lib)
    return out


def _norm_out(out: Optional[torch.Tensor], rows: int, D: int, device, dtype, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty((rows, D), device=device, dtype=dtype)
    _chk(out, dtype, name + ".out")
    if tuple(out.shape) != (rows, D):
        raise _lib.VitronHipError(f"{name}: out is {tuple(out.shape)}, expected {(rows, D)}")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, temb: Optional[torch.Tensor] = None,
              tokens_per_frame: int = 0, dtype=None, out: Optional[torch.Tensor] = None, rows: Optional[int] = None) -> torch.Tensor:
    """16-bit (`dtype`: bf16 default / fp16) LayerNorm of the fp32 rows of x; with temb ([T,D] fp32)
    x[row] += temb[(row//tokens_per_frame)%T] in place. `rows`: only the first `rows` rows of x; `out`: a contiguous [rows][D] tensor."""
    dtype = dtype or _lib.torch_dtype()
    lib = _lib.lib_for(dtype)
    _chk(x, torch.float32, "layernorm.x")
    D = x.shape[1]
    rows = x.shape[0] if rows is None else rows
    if not 0 < rows <= x.shape[0]:
        raise _lib.VitronHipError(f"layernorm: rows={rows} of an x of {x.shape[0]} rows")
    y = _norm_out(out, rows, D, x.device, dtype, "layernorm")
    T = 0 if temb is None else temb.shape[0]
    _lib.check(lib.vt_layernorm(_p(x), _p(temb), T, tokens_per_frame, _p(gamma), _p(beta), _p(y), rows, D, eps, _stream()),
               "vt_layernorm", lib)
    return y


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, idx: Optional[torch.Tensor] = None, dtype=None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dtype = dtype or _lib.torch_dtype()
    lib = _lib.lib_for(dtype)
    _chk(x, torch.float32, "rmsnorm.x")
    rows = x.shape[0] if idx is None else idx.shape[0]
    D = x.shape[1]
    y = _norm_out(out, rows, D, x.device, dtype, "rmsnorm")
    _lib.check(lib.vt_rmsnorm(_p(x), _p(idx), _p(w), _p(y), rows, D, eps, _stream()), "vt_rmsnorm", lib)
    return y


def seq_desc_tensor(rows: Sequence[Sequence[int]], device) -> torch.Tensor:
    """int32 [nseq,4] = (q_row0, q_len, kv_len, table_off)."""
    return torch.tensor(rows, dtype=torch.int32, device=device).reshape(-1, 4)


def kv_tiles(qkv: torch.Tensor, q_col0: int, k_col0: int, v_col0: int, k_tiles: torch.Tensor, vt_tiles: torch.Tensor,
             tile_table: torch.Tensor, seq_desc: torch.Tensor, max_new_tiles: int, heads: int, head_dim: int,
             rope_cos: Optional[torch.Tensor] = None, rope_sin: Optional[torch.Tensor] = None,
             positions: Optional[torch.Tensor] = None) -> None:
    lib, dt = _op16(qkv, "kv_tiles.qkv")
    _chk(qkv, dt, "kv_tiles.qkv")
    _chk(k_tiles, dt, "kv_tiles.k_tiles")
    if vt_tiles.element_size() != 2:        # fp16 bits in both builds; tests hand in raw 16-bit storage of either dtype
        raise _lib.VitronHipError("kv_tiles.vt_tiles: expected a 16-bit tensor (the V^T pages hold fp16 bits)")
    _lib.check(lib.vt_kv_tiles(_p(qkv), qkv.stride(0), q_col0, k_col0, v_col0, _p(k_tiles), _p(vt_tiles), _p(tile_table),
                               _p(seq_desc), seq_desc.shape[0], max_new_tiles, heads, head_dim, _p(rope_cos), _p(rope_sin),
                               _p(positions), _stream()), "vt_kv_tiles", lib)


def attn_tail_desc(seq_desc: torch.Tensor, logit_rows: torch.Tensor) -> torch.Tensor:
    """int32 [n,4]: the single-query descriptor of every logit row (vt_attn_tail_desc, include/vitron_hip.h), built on the device."""
    lib = _lib.load()
    n = logit_rows.numel()
    out = torch.empty((n, 4), dtype=torch.int32, device=seq_desc.device)
    _lib.check(lib.vt_attn_tail_desc(_p(seq_desc), seq_desc.shape[0], _p(logit_rows), n, _p(out), _stream()), "vt_attn_tail_desc", lib)
    return out


def flash_attn(q: torch.Tensor, k_tiles: torch.Tensor, vt_tiles: torch.Tensor, tile_table: torch.Tensor,
               seq_desc: torch.Tensor, max_q_len: int, heads: int, head_dim: int, causal: bool, scale: float,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q: bf16 [rows, ldq] view whose first heads*head_dim columns are the queries (e.g. the fused QKV buffer)."""
    lib, dt = _op16(q, "flash_attn.q")
    if k_tiles.dtype != dt:
        raise _lib.VitronHipError(f"flash_attn: q is {dt} but the K tiles are {k_tiles.dtype}")
    if out is None:
        out = torch.empty((q.shape[0], heads * head_dim), device=q.device, dtype=dt)
    _lib.check(lib.vt_flash_attn(_p(q), q.stride(0), _p(k_tiles), _p(vt_tiles), _p(tile_table), _p(seq_desc),
                                 seq_desc.shape[0], max_q_len, _p(out), out.stride(0), heads, head_dim, int(causal),
                                 float(scale), _stream()), "vt_flash_attn", lib)
    return out


def flash_attn_select(kernel: int) -> None:
    """Process-wide choice of the head_dim-128 prefill kernel in BOTH operand builds (vt_flash_attn_select, include/vitron_hip.h):
    0 automatic, 1 two-waves-per-SIMD kernel, 2 one-wave-per-SIMD hand-placed kernel, 3 that kernel unplaced (its reference), 4 the
    hand-placed kernel in its persistent form (4 | (n << 8): at most n workgroups), 5 kernel 2 in the grid's natural block order
    instead of the planned dispatch order."""
    for op in ("bf16", "fp16"):
        lib = _lib.load(operand=op)
        _lib.check(lib.vt_flash_attn_select(int(kernel)), "vt_flash_attn_select", lib)


def attn_decode(q: torch.Tensor, k_tiles: torch.Tensor, vt_tiles: torch.Tensor, tile_table: torch.Tensor,
                seq_desc: torch.Tensor, heads: int, head_dim: int, scale: float, max_kv_len: int) -> torch.Tensor:
    lib, dt = _op16(q, "attn_decode.q")
    out = torch.empty((q.shape[0], heads * head_dim), device=q.device, dtype=dt)
    nseq = seq_desc.shape[0]
    scratch = torch.empty(lib.vt_attn_decode_scratch_bytes(nseq, heads, head_dim, int(max_kv_len)), dtype=torch.uint8, device=q.device)
    _lib.check(lib.vt_attn_decode(_p(q), q.stride(0), _p(k_tiles), _p(vt_tiles), _p(tile_table), _p(seq_desc), nseq, _p(out),
                                  out.stride(0), heads, head_dim, float(scale), int(max_kv_len), _p(scratch), scratch.numel(),
                                  _stream()), "vt_attn_decode", lib)
    return out


def attn_decode_fused(qkv: torch.Tensor, q_col0: int, k_col0: int, v_col0: int, k_tiles: torch.Tensor, vt_tiles: torch.Tensor,
                      tile_table: torch.Tensor, seq_desc: torch.Tensor, heads: int, head_dim: int, scale: float,
                      rope_cos: Optional[torch.Tensor] = None, rope_sin: Optional[torch.Tensor] = None,
                      positions: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decode step's attention: rotary on the new q/k rows, k/v append to the paged tiles, attention, combine."""
    lib, dt = _op16(qkv, "attn_decode_fused.qkv")
    _chk(qkv, dt, "attn_decode_fused.qkv")
    _chk(k_tiles, dt, "attn_decode_fused.k_tiles")
    out = torch.empty((qkv.shape[0], heads * head_dim), device=qkv.device, dtype=dt)
    _lib.check(lib.vt_attn_decode_fused(_p(qkv), qkv.stride(0), q_col0, k_col0, v_col0, _p(k_tiles), _p(vt_tiles), _p(tile_table),
                                        _p(seq_desc), seq_desc.shape[0], _p(out), out.stride(0), heads, head_dim, float(scale),
                                        _p(rope_cos), _p(rope_sin), _p(positions), _stream()), "vt_attn_decode_fused", lib)
    return out


def _pages8(t: torch.Tensor, name: str):
    """fp8 (e4m3fn) pages travel as one byte per element: uint8 or torch.float8_e4m3fn storage."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitronHipError(f"{name}: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if t.element_size() != 1 or not t.is_contiguous():
        raise _lib.VitronHipError(f"{name}: expected contiguous 1-byte elements (e4m3 pages), got {t.dtype}")


def kv8_quant(k_tiles: torch.Tensor, vt_tiles: torch.Tensor, src_table: torch.Tensor, k8: torch.Tensor, vt8: torch.Tensor,
              dst_table: torch.Tensor, heads: int, head_dim: int) -> None:
    """Whole tiles: 16-bit tile src_table[i] of (k_tiles operand dtype, vt_tiles fp16 bits) -> e4m3 page dst_table[i] of (k8, vt8)."""
    lib, dt = _op16(k_tiles, "kv8_quant.k_tiles")
    _chk(k_tiles, dt, "kv8_quant.k_tiles")
    if vt_tiles.element_size() != 2 or not vt_tiles.is_contiguous():
        raise _lib.VitronHipError("kv8_quant.vt_tiles: expected a contiguous 16-bit tensor (the V^T pages hold fp16 bits)")
    _pages8(k8, "kv8_quant.k8")
    _pages8(vt8, "kv8_quant.vt8")
    _chk(src_table, torch.int32, "kv8_quant.src_table")
    _chk(dst_table, torch.int32, "kv8_quant.dst_table")
    if src_table.numel() != dst_table.numel():
        raise _lib.VitronHipError("kv8_quant: src_table and dst_table differ in length")
    tile = heads * PAGE_TOKENS * head_dim
    if src_table.numel() and (int(src_table.max()) + 1) * tile > k_tiles.numel() or src_table.numel() and (int(dst_table.max()) + 1) * tile > k8.numel():
        raise _lib.VitronHipError("kv8_quant: a table entry points past its pool")
    _lib.check(lib.vt_kv8_quant(_p(k_tiles), _p(vt_tiles), _p(src_table), _p(k8), _p(vt8), _p(dst_table), src_table.numel(), heads,
                                head_dim, _stream()), "vt_kv8_quant", lib)


def kv8_dequant(k8: torch.Tensor, vt8: torch.Tensor, src_table: torch.Tensor, k_tiles: torch.Tensor, vt_tiles: torch.Tensor,
                dst_table: torch.Tensor, heads: int, head_dim: int) -> None:
    """The inverse of kv8_quant (exact): e4m3 page src_table[i] -> 16-bit tile dst_table[i]."""
    lib, dt = _op16(k_tiles, "kv8_dequant.k_tiles")
    _chk(k_tiles, dt, "kv8_dequant.k_tiles")
    if vt_tiles.element_size() != 2 or not vt_tiles.is_contiguous():
        raise _lib.VitronHipError("kv8_dequant.vt_tiles: expected a contiguous 16-bit tensor (the V^T pages hold fp16 bits)")
    _pages8(k8, "kv8_dequant.k8")
    _pages8(vt8, "kv8_dequant.vt8")
    _chk(src_table, torch.int32, "kv8_dequant.src_table")
    _chk(dst_table, torch.int32, "kv8_dequant.dst_table")
    if src_table.numel() != dst_table.numel():
        raise _lib.VitronHipError("kv8_dequant: src_table and dst_table differ in length")
    tile = heads * PAGE_TOKENS * head_dim
    if src_table.numel() and (int(src_table.max()) + 1) * tile > k8.numel() or src_table.numel() and (int(dst_table.max()) + 1) * tile > k_tiles.numel():
        raise _lib.VitronHipError("kv8_dequant: a table entry points past its pool")
    _lib.check(lib.vt_kv8_dequant(_p(k8), _p(vt8), _p(src_table), _p(k_tiles), _p(vt_tiles), _p(dst_table), src_table.numel(), heads,
                                  head_dim, _stream()), "vt_kv8_dequant", lib)


def attn_decode_kv8(q: torch.Tensor, k8: torch.Tensor, vt8: torch.Tensor, tile_table: torch.Tensor, seq_desc: torch.Tensor,
                    heads: int, head_dim: int, scale: float, max_kv_len: int) -> torch.Tensor:
    """attn_decode on e4m3 pages."""
    lib, dt = _op16(q, "attn_decode_kv8.q")
    _pages8(k8, "attn_decode_kv8.k8")
    _pages8(vt8, "attn_decode_kv8.vt8")
    out = torch.empty((q.shape[0], heads * head_dim), device=q.device, dtype=dt)
    nseq = seq_desc.shape[0]
    scratch = torch.empty(lib.vt_attn_decode_scratch_bytes(nseq, heads, head_dim, int(max_kv_len)), dtype=torch.uint8, device=q.device)
    _lib.check(lib.vt_attn_decode_kv8(_p(q), q.stride(0), _p(k8), _p(vt8), _p(tile_table), _p(seq_desc), nseq, _p(out),
                                      out.stride(0), heads, head_dim, float(scale), int(max_kv_len), _p(scratch), scratch.numel(),
                                      _stream()), "vt_attn_decode_kv8", lib)
    return out


def attn_decode_fused_kv8(qkv: torch.Tensor, q_col0: int, k_col0: int, v_col0: int, k8: torch.Tensor, vt8: torch.Tensor,
                          tile_table: torch.Tensor, seq_desc: torch.Tensor, heads: int, head_dim: int, scale: float,
                          rope_cos: Optional[torch.Tensor] = None, rope_sin: Optional[torch.Tensor] = None,
                          positions: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attn_decode_fused on e4m3 pages: the new k row / v column are quantised, stored and scored from their quantised values."""
    lib, dt = _op16(qkv, "attn_decode_fused_kv8.qkv")
    _chk(qkv, dt, "attn_decode_fused_kv8.qkv")
    _pages8(k8, "attn_decode_fused_kv8.k8")
    _pages8(vt8, "attn_decode_fused_kv8.vt8")
    out = torch.empty((qkv.shape[0], heads * head_dim), device=qkv.device, dtype=dt)
    _lib.check(lib.vt_attn_decode_fused_kv8(_p(qkv), qkv.stride(0), q_col0, k_col0, v_col0, _p(k8), _p(vt8), _p(tile_table),
                                            _p(seq_desc), seq_desc.shape[0], _p(out), out.stride(0), heads, head_dim, float(scale),
                                            _p(rope_cos), _p(rope_sin), _p(positions), _stream()), "vt_attn_decode_fused_kv8", lib)
    return out


def attn_temporal(qkv: torch.Tensor, B: int, T: int, N: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib, dt = _op16(qkv, "attn_temporal.qkv")
    _chk(qkv, dt, "attn_temporal.qkv")
    if out is None:
        out = torch.empty((qkv.shape[0], heads * 64), device=qkv.device, dtype=dt)
    _chk(out, dt, "attn_temporal.out")
    if qkv.numel() < B * T * N * 3 * heads * 64 or out.numel() < B * T * N * heads * 64:
        raise _lib.VitronHipError(f"attn_temporal: qkv {tuple(qkv.shape)} / out {tuple(out.shape)} too small for {B * T * N} rows of {heads} heads")
    _lib.check(lib.vt_attn_temporal(_p(qkv), _p(out), B, T, N, heads, _stream()), "vt_attn_temporal", lib)
    return out


def attn_temporal_f32(qkv: torch.Tensor, B: int, T: int, N: int, heads: int, dtype=None, out: Optional[torch.Tensor] = None,
                      out_lo: Optional[torch.Tensor] = None):
    """Temporal attention on fp32 q | k | v rows (a row-strided view: its row stride travels as ld) -> (hi, lo), the output as an operand
    pair in `dtype` (default: the dtype of `out`, else the default operand)."""
    if dtype is None:
        dtype = out.dtype if out is not None else _lib.torch_dtype()
    lib = _lib.lib_for(dtype)
    _chk_view(qkv, torch.float32, "attn_temporal_f32.qkv")
    if qkv.dim() != 2 or qkv.shape[0] != B * T * N or qkv.shape[1] != 3 * heads * 64:
        raise _lib.VitronHipError(f"attn_temporal_f32: qkv is {tuple(qkv.shape)}, expected {(B * T * N, 3 * heads * 64)}")
    if out is None:
        out = torch.empty((qkv.shape[0], heads * 64), device=qkv.device, dtype=dtype)
    if out_lo is None:
        out_lo = torch.empty((qkv.shape[0], heads * 64), device=qkv.device, dtype=dtype)
    for name, t in (("out", out), ("out_lo", out_lo)):
        _chk(t, dtype, "attn_temporal_f32." + name)
        if t.numel() < B * T * N * heads * 64:
            raise _lib.VitronHipError(f"attn_temporal_f32.{name}: {t.numel()} elements for {B * T * N} rows of {heads * 64}")
    _lib.check(lib.vt_attn_temporal_f32(_p(qkv), qkv.stride(0), _p(out), _p(out_lo), B, T, N, heads, _stream()), "vt_attn_temporal_f32", lib)
    return out, out_lo


def vit_embed(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, g: torch.Tensor, b: torch.Tensor, F: int, G2: int,
              eps: float, out: Optional[torch.Tensor] = None, lib=None) -> torch.Tensor:
    """x fp32 [F * (G2 + 1)][D]: CLS / position add + pre-LayerNorm of the ViT front end (all fp32; `lib`: the build to run, default the
    default operand's -- the kernel has no 16-bit argument)."""
    lib = _lib.load() if lib is None else lib
    D = pos.shape[-1]
    for name, t, n in (("patch_out", patch_out, F * G2 * D), ("cls", cls, D), ("pos", pos, (G2 + 1) * D), ("g", g, D), ("b", b, D)):
        _chk(t, torch.float32, "vit_embed." + name)
        if t.numel() != n:
            raise _lib.VitronHipError(f"vit_embed.{name}: {t.numel()} elements, expected {n}")
    if out is None:
        out = torch.empty((F * (G2 + 1), D), device=pos.device, dtype=torch.float32)
    _chk(out, torch.float32, "vit_embed.out")
    if out.numel() < F * (G2 + 1) * D:
        raise _lib.VitronHipError(f"vit_embed.out: {out.numel()} elements for {F * (G2 + 1)} rows of {D}")
    _lib.check(lib.vt_vit_embed(_p(patch_out), _p(cls), _p(pos), _p(g), _p(b), _p(out), F, G2, D, float(eps), _stream()), "vt_vit_embed", lib)
    return out


def region_pool(feats: torch.Tensor, slices: torch.Tensor, G: int, image_size: int, pooled: Optional[torch.Tensor] = None,
                want_mask: bool = True, coords: Optional[torch.Tensor] = None, loc_w0: Optional[torch.Tensor] = None,
                loc_b0: Optional[torch.Tensor] = None, loc_out: Optional[torch.Tensor] = None,
                cell_mask: Optional[torch.Tensor] = None, cell_count: Optional[torch.Tensor] = None):
    """The pooling launch of the region extractor: feats 16-bit [B][G*G][D], slices int32 [B][4] -> (pooled [B][D], cell_mask int32
    [B][G*G] | None, cell_count int32 [B] | None, loc_out); want_mask=False passes NULL for the two optional outputs. With loc_out (a 16-bit [B][>= loc_n] tensor or row-strided view, loc_n =
    loc_w0.shape[0]) LocationEncoder layer 0 is evaluated into its first loc_n columns from coords fp32 [B][4], loc_w0 16-bit [loc_n][8]
    and loc_b0 fp32 [loc_n]."""
    lib, dt = _op16(feats, "region_pool.feats")
    _chk(feats, dt, "region_pool.feats")
    _chk(slices, torch.int32, "region_pool.slices")
    B = slices.shape[0]
    if feats.dim() != 3 or feats.shape[0] != B or feats.shape[1] != G * G or slices.numel() != B * 4:
        raise _lib.VitronHipError(f"region_pool: feats {tuple(feats.shape)} / slices {tuple(slices.shape)} do not describe {B} boxes on a {G}x{G} grid")
    D = feats.shape[2]
    if pooled is None:
        pooled = torch.empty((B, D), device=feats.device, dtype=dt)
    _chk(pooled, dt, "region_pool.pooled")
    if pooled.numel() < B * D:
        raise _lib.VitronHipError(f"region_pool.pooled: {pooled.numel()} elements for {B} rows of {D}")
    mask, count = cell_mask, cell_count
    if mask is None and want_mask:
        mask = torch.empty((B, G * G), device=feats.device, dtype=torch.int32)
    if count is None and want_mask:
        count = torch.empty((B,), device=feats.device, dtype=torch.int32)
    for name, t, n in (("cell_mask", mask, B * G * G), ("cell_count", count, B)):
        if t is not None:
            _chk(t, torch.int32, "region_pool." + name)
            if t.numel() < n:
                raise _lib.VitronHipError(f"region_pool.{name}: {t.numel()} elements, expected {n}")
    loc_n = ld_loc = 0
    if loc_out is not None:
        _chk_view(loc_out, dt, "region_pool.loc_out")
        _chk(coords, torch.float32, "region_pool.coords")
        _chk(loc_w0, dt, "region_pool.loc_w0")
        _chk(loc_b0, torch.float32, "region_pool.loc_b0")
        loc_n = loc_b0.numel()
        if loc_w0.numel() != loc_n * 8 or coords.numel() != B * 4 or loc_out.dim() != 2 or loc_out.shape[0] != B or loc_out.shape[1] < loc_n:
            raise _lib.VitronHipError(f"region_pool: loc_w0 {tuple(loc_w0.shape)} / coords {tuple(coords.shape)} / loc_out "
                                      f"{tuple(loc_out.shape)} do not describe {loc_n} outputs for {B} boxes")
        ld_loc = loc_out.stride(0)
    _lib.check(lib.vt_region_pool(_p(feats), _p(slices), B, G, image_size, D, _p(pooled), _p(mask), _p(count), _p(coords), _p(loc_w0),
                                  _p(loc_b0), loc_n, _p(loc_out), ld_loc, _stream()), "vt_region_pool", lib)
    return pooled, mask, count, loc_out


def im2col(pixels: torch.Tensor, patch: int, k_pad: int, dtype=None) -> torch.Tensor:
    """pixels fp32 or 16-bit; patches come out in `dtype` (default: the pixels' own 16-bit dtype, else the default operand)."""
    if dtype is None:
        dtype = pixels.dtype if pixels.dtype in (torch.bfloat16, torch.float16) else _lib.torch_dtype()
    lib = _lib.lib_for(dtype)
    if pixels.dtype not in (dtype, torch.float32):
        raise _lib.VitronHipError(f"im2col: pixels are {pixels.dtype}, expected {dtype} or fp32")
    video = pixels.dim() == 5
    if video:
        B, _, T, H, W = pixels.shape
    else:
        B, _, H, W = pixels.shape
        T = 1
    dt = _lib.DTYPE_F32 if pixels.dtype == torch.float32 else _lib.DTYPE_BF16
    out = torch.empty((B * T * (H // patch) * (W // patch), k_pad), device=pixels.device, dtype=dtype)
    _lib.check(lib.vt_im2col(_p(pixels.contiguous()), dt, _p(out), B, T, H, W, patch, k_pad, int(video), _stream()), "vt_im2col", lib)
    return out


def _chk_rows(t: torch.Tensor, dtype, name: str):
    """2-D tensor whose rows are contiguous (row stride free): logits narrowed to the true vocabulary of a padded lm_head."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitronHipError(f"{name}: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
        raise _lib.VitronHipError(f"{name}: expected a 2-D {dtype} tensor with contiguous rows")


def embed_splice(tok_table: torch.Tensor, vis: Optional[torch.Tensor], reg: Optional[torch.Tensor], plan: torch.Tensor) -> torch.Tensor:
    lib, dt = _op16(tok_table, "embed_splice.tok_table")
    _chk(tok_table, dt, "embed_splice.tok_table")
    for name, t in (("vis", vis), ("reg", reg)):
        if t is not None and t.dtype != dt:
            raise _lib.VitronHipError(f"embed_splice.{name}: {t.dtype} rows cannot be spliced into a {dt} sequence")
    rows, H = plan.shape[0], tok_table.shape[1]
    out = torch.empty((rows, H), device=tok_table.device, dtype=dt)
    _lib.check(lib.vt_embed_splice(_p(tok_table), tok_table.shape[0], _p(vis), 0 if vis is None else vis.shape[0], _p(reg),
                                   0 if reg is None else reg.shape[0], _p(plan), rows, H, _p(out), _stream()), "vt_embed_splice", lib)
    return out


def argmax(logits: torch.Tensor) -> torch.Tensor:
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "argmax.logits")
    rows, V = logits.shape
    out = torch.empty((rows,), device=logits.device, dtype=torch.int32)
    _lib.check(lib.vt_argmax(_p(logits), rows, V, logits.stride(0), _p(out), _stream()), "vt_argmax", lib)
    return out


def decode_feed(tok_table: torch.Tensor, next_ids: torch.Tensor, finished: torch.Tensor, eos_ids: Optional[torch.Tensor],
                pad_id: int, tokens_out: torch.Tensor, x: torch.Tensor, seq_desc: torch.Tensor, positions: torch.Tensor) -> None:
    """In-place decode-loop feedback (vt_decode_feed): token resolution, EOS flags, next input rows, metadata advance."""
    lib, dt = _op16(tok_table, "decode_feed.tok_table")
    _chk(tok_table, dt, "decode_feed.tok_table")
    _chk(x, dt, "decode_feed.x")
    for name, t in (("next_ids", next_ids), ("finished", finished), ("tokens_out", tokens_out), ("seq_desc", seq_desc),
                    ("positions", positions)):
        _chk(t, torch.int32, f"decode_feed.{name}")
    nseq = next_ids.shape[0]
    if finished.numel() != nseq or tokens_out.numel() != 2 * nseq or seq_desc.numel() != 4 * nseq or positions.numel() != nseq \
            or tuple(x.shape) != (nseq, tok_table.shape[1]):
        raise _lib.VitronHipError("decode_feed: buffer sizes do not match the number of sequences")
    n_eos = 0 if eos_ids is None else int(eos_ids.numel())
    if n_eos:
        _chk(eos_ids, torch.int32, "decode_feed.eos_ids")
    _lib.check(lib.vt_decode_feed(_p(tok_table), tok_table.shape[1], tok_table.shape[0], _p(next_ids), _p(finished),
                                  _p(eos_ids) if n_eos else None, n_eos, int(pad_id), _p(tokens_out), _p(x), _p(seq_desc),
                                  _p(positions), nseq, _stream()), "vt_decode_feed", lib)


def sample_top_p(logits: torch.Tensor, temperature: float, top_p: float, seed: int, step: int, return_kept: bool = False,
                 top_k: int = 0):
    """One sampled token id per row (int32), on device; see vt_sample_top_p in include/vitron_hip.h."""
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "sample_top_p.logits")
    rows, V = logits.shape
    out = torch.empty((rows,), device=logits.device, dtype=torch.int32)
    kept = torch.empty((rows,), device=logits.device, dtype=torch.int32) if return_kept else None
    _lib.check(lib.vt_sample_top_p(_p(logits), rows, V, logits.stride(0), float(temperature), int(top_k or 0),
                                   float(top_p if top_p else 1.0), int(seed) & (2 ** 64 - 1), int(step), _p(out), _p(kept),
                                   _stream()), "vt_sample_top_p", lib)
    return (out, kept) if return_kept else out


def _row_pointers(what: str, entries, rows: int, device, kind: str, ok, want: str) -> torch.Tensor:
    """int64 [rows] on `device`: the data pointer of each entry, 0 for None. Every other entry is a contiguous tensor on `device` that
    passes ok(); `kind` and `want` word the two refusals. One small host -> device copy."""
    if isinstance(entries, torch.Tensor) or not hasattr(entries, "__len__") or len(entries) != rows:
        raise _lib.VitronHipError(f"sample_rows.{what}: expected a sequence of {rows} entries (one per row), each None or {kind}")
    ptrs = []
    for i, m in enumerate(entries):
        if m is not None and not (isinstance(m, torch.Tensor) and m.device == device and m.is_contiguous() and ok(m)):
            raise _lib.VitronHipError(f"sample_rows.{what}[{i}]: expected None or {want} on the logits' device")
        ptrs.append(0 if m is None else m.data_ptr())
    return torch.tensor(ptrs, dtype=torch.int64).to(device)


def allow_pointers(allow, rows: int, V: int, device) -> torch.Tensor:
    """The device pointer array vt_sample_rows_allow reads (int64 [rows]) from one entry per row: None (NULL: everything allowed) or a
    contiguous int32 / uint32 device tensor of ceil(V / 32) mask words (sampling.allow_mask). The caller keeps the masks alive until
    the launch has run. One small host -> device copy."""
    words = (V + 31) // 32
    mask_dtypes = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
    return _row_pointers("allow", allow, rows, device, "a mask tensor", lambda m: m.dtype in mask_dtypes and m.numel() == words,
                         f"a contiguous int32 / uint32 tensor of {words} words (ceil(V / 32), V = {V})")


def adjust_pointers(adjust, rows: int, V: int, device) -> torch.Tensor:
    """The device pointer array vt_sample_rows_adj reads (int64 [rows]) from one entry per row: None (NULL: no adjustment) or a
    contiguous fp32 device tensor of 2 * V elements, the (pre, post) pairs ops.bias_rows writes. The caller keeps the buffers alive until
    the launch has run. One small host -> device copy."""
    return _row_pointers("adjust", adjust, rows, device, "an fp32 tensor",
                         lambda m: m.dtype == torch.float32 and m.numel() == 2 * V and m.data_ptr() % 8 == 0,
                         f"a contiguous, 8-byte aligned fp32 tensor of {2 * V} elements ([V][2], V = {V})")


def sample_rows(logits: torch.Tensor, params: torch.Tensor, return_kept: bool = False, return_logprob: bool = False, allow=None,
                _allow_ptrs: Optional[torch.Tensor] = None, adjust=None, _adjust_ptrs: Optional[torch.Tensor] = None,
                trunc: Optional[torch.Tensor] = None, watermark: Optional[torch.Tensor] = None, miro: Optional[torch.Tensor] = None):
    """One token id per row (int32, on device) with PER-ROW parameters: greedy and sampled rows, penalties and the chosen token's
    log-probability in one launch; see vt_sample_rows in include/vitron_hip.h. `params`: the device array of vt_sample_row that
    sampling.pack_sample_rows builds (uint8 [rows, 48]). Returns ids, or (ids[, kept_count][, logprob]) when either is asked for.
    allow: per-row allow masks (vt_sample_rows_allow) -- a sequence of `rows` entries, each None or a device tensor of ceil(V / 32)
    mask words; each is checked and the pointer array is built here. None: today's vt_sample_rows call.
    _allow_ptrs (private; generate's single upload, tools/sampler_bench.py): a pointer array that allow_pointers -- or its caller, from
    masks it has checked itself -- built earlier, int64 [rows]; its values are dereferenced on the device as they are.
    adjust: per-row additive adjustments (vt_sample_rows_adj) -- a sequence of `rows` entries, each None or a device fp32 tensor of
    2 * V elements, the (pre, post) pairs of ops.bias_rows; pre is added before the repetition penalty, post after it. _adjust_ptrs is
    its private pointer-array form, like _allow_ptrs. With neither, the launches are the ones above.
    trunc: per-row truncation (vt_sample_rows_trunc: min_p, typical_p, epsilon_cutoff, eta_cutoff after top-k and top-p) -- the device
    array of vt_trunc_row that sampling.pack_trunc_rows builds (uint8, rows x 16 bytes). None: exactly the calls above.
    watermark: per-row SynthID text watermark (vt_sample_rows_wm, DESIGN.md 9.16: the tournament behind the truncation stages, the
    sequences' state on the device) -- the device array of vt_wm_row that watermark.pack_wm_rows builds (uint8, rows x 48 bytes).
    None: exactly the calls above.
    miro: per-row Mirostat v2 (vt_sample_rows_miro, DESIGN.md 9.17: the moving surprise cutoff behind the truncation stages, the
    sequences' {mu, last_surprise} cells on the device) -- the device array of vt_miro_row that sampling.pack_miro_rows builds (uint8,
    rows x 16 bytes). None: exactly the calls above. Together with `watermark` it is refused: that kernel is not built."""
    from .sampling import MIRO_ROW_BYTES, ROW_BYTES, TRUNC_ROW_BYTES
    from .watermark import WM_ROW_BYTES
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "sample_rows.logits")
    rows, V = logits.shape
    if not isinstance(params, torch.Tensor) or params.device != logits.device or params.dtype != torch.uint8 \
            or not params.is_contiguous() or params.numel() != rows * ROW_BYTES:
        raise _lib.VitronHipError(f"sample_rows.params: expected a contiguous uint8 tensor of {rows} x {ROW_BYTES} bytes on the logits' device "
                                  "(sampling.pack_sample_rows)")
    out = torch.empty((rows,), device=logits.device, dtype=torch.int32)
    kept = torch.empty((rows,), device=logits.device, dtype=torch.int32) if return_kept else None
    lp = torch.empty((rows,), device=logits.device, dtype=torch.float32) if return_logprob else None
    if allow is not None and _allow_ptrs is not None:
        raise _lib.VitronHipError("sample_rows: pass allow or _allow_ptrs, not both")
    if adjust is not None and _adjust_ptrs is not None:
        raise _lib.VitronHipError("sample_rows: pass adjust or _adjust_ptrs, not both")

    def given_ptrs(ptrs, what):
        if not isinstance(ptrs, torch.Tensor) or ptrs.dtype != torch.int64 or ptrs.device != logits.device or not ptrs.is_contiguous() \
                or ptrs.numel() != rows:
            raise _lib.VitronHipError(f"sample_rows.{what}: expected a contiguous int64 [{rows}] tensor on the logits' device")
        return ptrs
    if trunc is not None and (not isinstance(trunc, torch.Tensor) or trunc.device != logits.device or trunc.dtype != torch.uint8
                              or not trunc.is_contiguous() or trunc.numel() != rows * TRUNC_ROW_BYTES):
        raise _lib.VitronHipError(f"sample_rows.trunc: expected a contiguous uint8 tensor of {rows} x {TRUNC_ROW_BYTES} bytes on the logits' "
                                  "device (sampling.pack_trunc_rows)")
    if watermark is not None and (not isinstance(watermark, torch.Tensor) or watermark.device != logits.device
                                  or watermark.dtype != torch.uint8 or not watermark.is_contiguous()
                                  or watermark.numel() != rows * WM_ROW_BYTES):
        raise _lib.VitronHipError(f"sample_rows.watermark: expected a contiguous uint8 tensor of {rows} x {WM_ROW_BYTES} bytes on the "
                                  "logits' device (watermark.pack_wm_rows)")
    if miro is not None and (not isinstance(miro, torch.Tensor) or miro.device != logits.device or miro.dtype != torch.uint8
                             or not miro.is_contiguous() or miro.numel() != rows * MIRO_ROW_BYTES):
        raise _lib.VitronHipError(f"sample_rows.miro: expected a contiguous uint8 tensor of {rows} x {MIRO_ROW_BYTES} bytes on the logits' "
                                  "device (sampling.pack_miro_rows)")
    if miro is not None and watermark is not None:
        raise _lib.VitronHipError("sample_rows: miro together with watermark is not built (vt_sample_rows_miro carries no watermark)")
    aptrs = given_ptrs(_allow_ptrs, "_allow_ptrs") if _allow_ptrs is not None else \
        None if allow is None else allow_pointers(allow, rows, V, logits.device)
    jptrs = given_ptrs(_adjust_ptrs, "_adjust_ptrs") if _adjust_ptrs is not None else \
        None if adjust is None else adjust_pointers(adjust, rows, V, logits.device)
    # the narrowest entry point that carries what was given: error texts name it, and the library picks the kernel by the same rule
    if miro is not None:
        name, extra = "vt_sample_rows_miro", (aptrs, jptrs, trunc, miro)
    elif watermark is not None:
        name, extra = "vt_sample_rows_wm", (aptrs, jptrs, trunc, watermark)
    elif trunc is not None:
        name, extra = "vt_sample_rows_trunc", (aptrs, jptrs, trunc)
    elif jptrs is not None:
        name, extra = "vt_sample_rows_adj", (aptrs, jptrs)
    elif aptrs is not None:
        name, extra = "vt_sample_rows_allow", (aptrs,)
    else:
        name, extra = "vt_sample_rows", ()
    _lib.check(getattr(lib, name)(_p(logits), rows, V, logits.stride(0), _p(params), *map(_p, extra), _p(out), _p(kept), _p(lp),
                                  _stream()), name, lib)
    res = (out,) + ((kept,) if return_kept else ()) + ((lp,) if return_logprob else ())
    return res if len(res) > 1 else out


def _launch_rows(name: str, row_bytes: int, rows_dev: Optional[torch.Tensor], n_rows: int, V: int, none_ok: bool = False) -> None:
    """The launch behind ban_rows, fsm_rows, cfg_rows, dola_rows and bias_rows: vt_<name>_rows over the device array of vt_<name>_row that
    sampling.pack_<name>_rows builds. rows_dev reaches the library as NULL when n_rows <= 0, or (none_ok: the cfg / dola rule) exactly
    when it is None, so that the library states what is wrong with the call."""
    lib = _lib.load_any()
    n_rows = int(n_rows)
    given = rows_dev is not None if none_ok else n_rows > 0
    if given and n_rows > 0:
        _chk(rows_dev, torch.uint8, f"{name}_rows.rows_dev")
        if rows_dev.numel() != n_rows * row_bytes:
            raise _lib.VitronHipError(f"{name}_rows.rows_dev: expected {n_rows} x {row_bytes} bytes (sampling.pack_{name}_rows), got "
                                      f"{rows_dev.numel()}")
    _lib.check(getattr(lib, f"vt_{name}_rows")(_p(rows_dev) if given else None, n_rows, int(V), _stream()), f"vt_{name}_rows", lib)


def ban_rows(rows_dev: torch.Tensor, n_rows: int, V: int) -> None:
    """Build the allow masks of n_rows rows on the device from their histories (n-gram and word-sequence bans); see vt_ban_rows in
    include/vitron_hip.h. rows_dev: the device array of vt_ban_row that sampling.pack_ban_rows builds (contiguous uint8, n_rows x 48
    bytes). Every pointer inside it is dereferenced on the device as it is: the caller keeps the buffers alive until the launch has
    run, sizes every `out` and `base` for ceil(V / 32) words, and lets no `out` alias a `base` or another `out`."""
    from .sampling import BAN_ROW_BYTES
    _launch_rows("ban", BAN_ROW_BYTES, rows_dev, n_rows, V)


def fsm_rows(rows_dev: torch.Tensor, n_rows: int, V: int) -> None:
    """Advance the automaton states of n_rows rows over the ids they have generated and build their allow masks on the device (guided
    decoding); see vt_fsm_rows in include/vitron_hip.h. rows_dev: the device array of vt_fsm_row that sampling.pack_fsm_rows builds
    (contiguous uint8, n_rows x 96 bytes). Every pointer inside it is dereferenced on the device as it is: the caller keeps the buffers
    alive until the launch has run, sizes every `out` and `base` for ceil(V / 32) words, gives every row its own two-int cell and lets
    no `out` alias a `base` or another `out`."""
    from .sampling import FSM_ROW_BYTES
    _launch_rows("fsm", FSM_ROW_BYTES, rows_dev, n_rows, V)


def cfg_rows(rows_dev: Optional[torch.Tensor], n_rows: int, V: int) -> None:
    """Classifier-free guidance over n_rows logit rows on the device: out = ul + scale * (cl - ul) from the log-softmaxes of a conditional
    and an unconditional row, optionally the plausibility mask and the two lse values; see vt_cfg_rows in include/vitron_hip.h. rows_dev:
    the device array of vt_cfg_row that sampling.pack_cfg_rows builds (contiguous uint8, n_rows x 56 bytes). Every pointer inside it is
    dereferenced on the device as it is: the caller keeps the buffers alive until the launch has run, sizes `cond`, `uncond` and `out`
    for V floats and `base` / `mask_out` for ceil(V / 32) words; `out` may be `cond` itself and nothing else that the launch reads."""
    from .sampling import CFG_ROW_BYTES
    _launch_rows("cfg", CFG_ROW_BYTES, rows_dev, n_rows, V, none_ok=True)


def dola_rows(rows_dev: Optional[torch.Tensor], n_rows: int, V: int) -> None:
    """DoLa over n_rows logit rows on the device: per row the candidate layer furthest from the final one and out = log_softmax(final) -
    log_softmax(candidate) over the tokens final >= max(final) + log_relative_top, -inf elsewhere; optionally the mask of the kept tokens,
    the chosen index, the divergences and the lse values; see vt_dola_rows in include/vitron_hip.h. rows_dev: the device array of
    vt_dola_row that sampling.pack_dola_rows builds (contiguous uint8, n_rows x 80 bytes). Every pointer inside it is dereferenced on the
    device as it is: the caller keeps the buffers alive until the launch has run; `out` may be `final` itself and nothing else that the
    launch reads."""
    from .sampling import DOLA_ROW_BYTES
    _launch_rows("dola", DOLA_ROW_BYTES, rows_dev, n_rows, V, none_ok=True)


def bias_rows(rows_dev: torch.Tensor, n_rows: int, V: int) -> None:
    """Build the additive adjustments of n_rows rows on the device (logit bias, presence and frequency penalties over the generated
    ids); see vt_bias_rows in include/vitron_hip.h. rows_dev: the device array of vt_bias_row that sampling.pack_bias_rows builds
    (contiguous uint8, n_rows x 48 bytes). Every pointer inside it is dereferenced on the device as it is: the caller keeps the
    buffers alive until the launch has run, sizes every `out` for 2 * V floats and lets no `out` alias another."""
    from .sampling import BIAS_ROW_BYTES
    _launch_rows("bias", BIAS_ROW_BYTES, rows_dev, n_rows, V)


def beam_step(logits: torch.Tensor, beam_scores: torch.Tensor, groups: int, beams_in: int, n_out: int, packed: bool = False):
    """The n_out best continuations of every beam group, on the device; see vt_beam_step in include/vitron_hip.h. logits: fp32
    [groups * beams_in, V] with contiguous rows (row g * beams_in + b: beam b of group g), beam_scores: fp32 [groups * beams_in].
    Returns (scores fp32, tokens int32, beams int32), each [groups, n_out], in descending score; exact ties by the lower b * V + t.
    packed=True returns the one int32 tensor [3, groups, n_out] behind them instead (the scores as their bits): one read-back.
    The limits (beams_in <= 16, n_out <= 32, n_out <= V) are the library's and raise through it."""
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "beam_step.logits")
    rows, V = logits.shape
    groups, beams_in, n_out = int(groups), int(beams_in), int(n_out)
    if groups < 1 or beams_in < 1 or rows != groups * beams_in:
        raise _lib.VitronHipError(f"beam_step: logits has {rows} rows, groups * beams_in = {groups} * {beams_in}")
    if not isinstance(beam_scores, torch.Tensor) or beam_scores.device != logits.device or beam_scores.dtype != torch.float32 \
            or not beam_scores.is_contiguous() or beam_scores.numel() != rows:
        raise _lib.VitronHipError(f"beam_step.beam_scores: expected a contiguous fp32 tensor of {rows} values on the logits' device")
    dev = logits.device
    # one allocation: the three outputs [3][groups][n_out], then the scratch
    n_res = 3 * groups * max(n_out, 0)
    nbytes = int(lib.vt_beam_step_scratch_bytes(groups, beams_in, n_out))
    buf = torch.empty((n_res + (nbytes + 3) // 4,), device=dev, dtype=torch.int32)
    res = buf[:n_res].view(3, groups, max(n_out, 0))
    base = buf.data_ptr()
    plane = 4 * groups * max(n_out, 0)
    _lib.check(lib.vt_beam_step(_p(logits), logits.stride(0), V, groups, beams_in, _p(beam_scores), n_out, base, base + plane,
                                base + 2 * plane, base + 3 * plane, nbytes, _stream()), "vt_beam_step", lib)
    if packed:
        return res
    return res[0].view(torch.float32), res[1], res[2]


LOGPROB_MAX_TOP = 20               # VT_LOGPROB_MAX_TOP


def logprob_rows(logits: torch.Tensor, targets: Optional[torch.Tensor] = None, n_top: int = 0, return_rank: bool = False,
                 return_lse: bool = False, out: Optional[dict] = None) -> dict:
    """Log-probabilities of RAW logit rows on the device, one launch; see vt_logprob_rows in include/vitron_hip.h. logits: fp32 [rows, V]
    with contiguous rows (row stride free). targets: int32 [rows] on the logits' device (an id outside [0, V) marks a row without a
    target), or None. Returns a dict of device tensors holding what was asked for:
      "logprob" fp32 [rows]           the targets' log-probabilities (NaN where a row has no target)         -- with targets
      "rank"    int32 [rows]          1 + the number of tokens strictly ahead of the target (0: no target)    -- with targets and return_rank
      "lse"     fp32 [rows]           the rows' log-sum-exp                                                   -- with return_lse
      "top_ids" int32 [rows, n_top], "top_logprobs" fp32 [rows, n_top]   larger logit first, ties by the lower id; (-1, NaN) where a
                                      row holds fewer than n_top takeable values                              -- with n_top > 0
    out: a dict with preallocated tensors under those keys (contiguous, of exactly those shapes and dtypes, on the logits' device --
    e.g. step s of [T, rows, n_top] buffers). Its keys then SAY what is computed -- the flags are not consulted; n_top > 0 needs both
    top keys -- and the kernel writes into them: nothing is allocated and nothing waits. Without `out` everything comes from ONE
    allocation (also returned as "packed", int32: the planes logprob, rank, lse, top_ids, top_logprobs in that order, those asked
    for), so a caller can read all of it back with one copy."""
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "logprob_rows.logits")
    rows, V = logits.shape
    n_top = int(n_top)
    if not 0 <= n_top <= LOGPROB_MAX_TOP:
        raise _lib.VitronHipError(f"logprob_rows: n_top={n_top} (0 <= n_top <= {LOGPROB_MAX_TOP})")
    dev = logits.device
    if targets is not None:
        _chk(targets, torch.int32, "logprob_rows.targets")
        if targets.device != dev or targets.numel() != rows:
            raise _lib.VitronHipError(f"logprob_rows.targets: expected int32 [{rows}] on the logits' device")
    out = {} if out is None else out
    unknown = set(out) - {"logprob", "rank", "lse", "top_ids", "top_logprobs"}
    if unknown:
        raise _lib.VitronHipError(f"logprob_rows.out: unknown key(s) {sorted(unknown)}")
    if out:
        want = {k: k in out for k in ("logprob", "rank", "lse")}
        want["top_ids"] = want["top_logprobs"] = n_top > 0
    else:
        want = {"logprob": targets is not None, "rank": targets is not None and bool(return_rank), "lse": bool(return_lse),
                "top_ids": n_top > 0, "top_logprobs": n_top > 0}
    spec = {"logprob": ((rows,), torch.float32), "rank": ((rows,), torch.int32), "lse": ((rows,), torch.float32),
            "top_ids": ((rows, n_top), torch.int32), "top_logprobs": ((rows, n_top), torch.float32)}
    if not any(want.values()):
        raise _lib.VitronHipError("logprob_rows: nothing asked for (no targets, n_top = 0, no lse)")
    res = {}
    for key, t in out.items():
        shape, dtype = spec[key]
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.VitronHipError(f"logprob_rows.out[{key!r}]: expected a contiguous {dtype} tensor of shape {shape} on the logits' device")
        if want[key]:
            res[key] = t
    missing = [k for k in spec if want[k] and k not in res]
    if out and missing:
        raise _lib.VitronHipError(f"logprob_rows.out: n_top={n_top} needs preallocated {missing}")
    if missing:                                  # (no `out`: everything in one allocation)
        sizes = [rows * (n_top if k.startswith("top_") else 1) for k in missing]
        buf = torch.empty((sum(sizes),), device=dev, dtype=torch.int32)
        at = 0
        for k, n in zip(missing, sizes):
            shape, dtype = spec[k]
            res[k] = buf[at:at + n].view(dtype).view(shape)
            at += n
        res["packed"] = buf
    _lib.check(lib.vt_logprob_rows(_p(logits), rows, V, logits.stride(0), _p(targets), n_top, _p(res.get("lse")), _p(res.get("logprob")),
                                   _p(res.get("rank")), _p(res.get("top_ids")), _p(res.get("top_logprobs")), _stream()),
               "vt_logprob_rows", lib)
    return res


CONTRAST_MAX_K = 16                # VT_CONTRAST_MAX_K
CONTRAST_CHUNK = 16                # VT_CONTRAST_CHUNK


def unit_rows(x: torch.Tensor, w: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """out[r] = (w * x[r]) / |w * x[r]| in the operand format, the norm and the products in fp32 (a zero row gives zeros); see vt_unit_rows in
    include/vitron_hip.h. x: fp32 [rows, H], contiguous or a row-strided view. w: fp32 [H] or None. out: a bf16 / fp16 [rows, H] tensor or
    row-strided view to write (e.g. rows of a context bank) -- its dtype picks the library build; without it a new tensor of `dtype`."""
    _chk_view(x, torch.float32, "unit_rows.x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise _lib.VitronHipError(f"unit_rows.x: expected fp32 [rows, H] with rows, H >= 1, got {tuple(x.shape)}")
    rows, H = x.shape
    if w is not None:
        _chk(w, torch.float32, "unit_rows.w")
        if w.numel() != H or w.device != x.device:
            raise _lib.VitronHipError(f"unit_rows.w: expected fp32 [{H}] on x's device, got {tuple(w.shape)}")
    if out is None:
        if dtype is None:
            raise _lib.VitronHipError("unit_rows: give out or dtype (bf16 / fp16)")
        out = torch.empty((rows, H), dtype=dtype, device=x.device)
    lib, dt = _op16(out, "unit_rows.out")
    _chk_view(out, dt, "unit_rows.out")
    if tuple(out.shape) != (rows, H) or out.device != x.device:
        raise _lib.VitronHipError(f"unit_rows.out: expected [{rows}, {H}] on x's device, got {tuple(out.shape)}")
    _lib.check(lib.vt_unit_rows(_p(x), x.stride(0) if rows > 1 else H, _p(w), _p(out), out.stride(0) if rows > 1 else H, rows, H, _stream()),
               "vt_unit_rows", lib)
    return out


def contrast_workspace(n_groups: int, max_bank_len: int, device) -> torch.Tensor:
    """A workspace for contrast_rows: VT_CONTRAST_WORKSPACE_BYTES(n_groups, max_bank_len) as fp32."""
    return torch.empty((max(int(n_groups), 1) * ((max(int(max_bank_len), 1) + CONTRAST_CHUNK - 1) // CONTRAST_CHUNK) * 16,),
                       dtype=torch.float32, device=device)


def contrast_rows(groups: Sequence[dict], cand: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> None:
    """The selection step of contrastive search for len(groups) sequences, on the device; see vt_contrast_rows in include/vitron_hip.h.
    cand: bf16 / fp16 [n_cand, H] unit rows (unit_rows), contiguous or row-strided. Each group is a dict:
      "bank"      bf16 / fp16 [cap, H] contiguous, cand's dtype: the context's unit rows in [0, bank_len); row bank_len is WRITTEN
      "bank_len"  T, 1 <= T < cap          "k" in [1, 16]          "first": the group's candidates are cand[first : first + k]
      "alpha"     in [0, 1]                "lp" fp32, at least k contiguous values: the candidates' log-probabilities
      "d", "score" fp32 [>= k], "sel" int32 [>= 1]: written (contiguous)
    Per candidate d = max_j dot(bank[j], cand), score = (1 - alpha) exp(lp) - alpha d; sel = the arg-max of the scores, ties to the lower
    candidate; bank[T] = cand[first + sel]. The row array stays on the host (nothing is uploaded); shapes are checked here, values by the
    launcher. workspace: fp32, contrast_workspace(len(groups), max T) elements; allocated when None."""
    lib, dt = _op16(cand, "contrast_rows.cand")
    _chk_view(cand, dt, "contrast_rows.cand")
    if cand.dim() != 2:
        raise _lib.VitronHipError(f"contrast_rows.cand: expected [n_cand, H], got {tuple(cand.shape)}")
    n_cand, H = cand.shape
    n = len(groups)
    if n < 1:
        raise _lib.VitronHipError("contrast_rows: no groups")
    arr = (_lib.VtContrastRow * n)()
    max_T = 1
    for g, grp in enumerate(groups):
        bank, k = grp["bank"], int(grp["k"])
        _chk(bank, dt, f"contrast_rows.groups[{g}].bank")
        if bank.dim() != 2 or bank.shape[1] != H or bank.device != cand.device:
            raise _lib.VitronHipError(f"contrast_rows.groups[{g}].bank: expected [cap, {H}] on cand's device, got {tuple(bank.shape)}")
        for key, tdt, need in (("lp", torch.float32, k), ("d", torch.float32, k), ("score", torch.float32, k), ("sel", torch.int32, 1)):
            t = grp[key]
            _chk(t, tdt, f"contrast_rows.groups[{g}].{key}")
            if t.numel() < max(need, 1) or t.device != cand.device:
                raise _lib.VitronHipError(f"contrast_rows.groups[{g}].{key}: expected at least {need} elements on cand's device, got {t.numel()}")
        r = arr[g]
        r.bank, r.cand_lp, r.d_out, r.score_out, r.sel_out = _p(bank), _p(grp["lp"]), _p(grp["d"]), _p(grp["score"]), _p(grp["sel"])
        r.bank_len, r.bank_cap, r.k, r.first, r.alpha, r.reserved = int(grp["bank_len"]), bank.shape[0], k, int(grp["first"]), float(grp["alpha"]), 0
        max_T = max(max_T, int(grp["bank_len"]))
    if workspace is None:
        workspace = contrast_workspace(n, max_T, cand.device)
    _chk(workspace, torch.float32, "contrast_rows.workspace")
    if workspace.device != cand.device:
        raise _lib.VitronHipError("contrast_rows.workspace: expected a tensor on cand's device")
    _lib.check(lib.vt_contrast_rows(arr, n, _p(cand), n_cand, cand.stride(0) if n_cand > 1 else H, H, _p(workspace), workspace.numel() * 4,
                                    _stream()), "vt_contrast_rows", lib)


def kv_copy_pages(kv, src_pages, dst_pages) -> None:
    """Copy page src_pages[i] onto page dst_pages[i] of a PagedKVCache, in every layer and both pools (vt_kv_copy_pages; either pool
    format). The ids are host sequences: each is checked against the pool here, and no destination may also be a source."""
    lib = _lib.load_any()
    src = [int(p) for p in src_pages]
    dst = [int(p) for p in dst_pages]
    if len(src) != len(dst):
        raise _lib.VitronHipError(f"kv_copy_pages: {len(src)} sources, {len(dst)} destinations")
    for name, ids in (("src_pages", src), ("dst_pages", dst)):
        for p in ids:
            if not 0 <= p < kv.num_pages:
                raise _lib.VitronHipError(f"kv_copy_pages.{name}: page {p} outside the pool of {kv.num_pages} pages")
    if set(src) & set(dst) or len(set(dst)) != len(dst):
        raise _lib.VitronHipError("kv_copy_pages: a destination page is also a source, or is written twice")
    if not src:
        return
    llama = kv.llama
    page_bytes = llama.heads * 64 * llama.hd * kv.k.element_size()
    if kv.vt.element_size() != kv.k.element_size():
        raise _lib.VitronHipError("kv_copy_pages: the K and V^T pools differ in element size")
    ids = torch.tensor([src, dst], dtype=torch.int32).to(kv.k.device)
    _lib.check(lib.vt_kv_copy_pages(_p(kv.k), _p(kv.vt), llama.L, kv.num_pages, page_bytes, _p(ids[0]), _p(ids[1]), len(src), _stream()),
               "vt_kv_copy_pages", lib)


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """Mean cross entropy of fp32 logits [rows, V] against int labels [rows] (rows with `ignore_index` skipped); 0-dim tensor."""
    lib = _lib.load_any()
    _chk_rows(logits, torch.float32, "cross_entropy.logits")
    rows, V = logits.shape
    lab = labels.to(device=logits.device, dtype=torch.int32).contiguous()
    # torch.nn.functional.cross_entropy raises on a label outside [0, V) that is not ignore_index; the kernel would drop such a
    # row from the mean, i.e. turn a vocabulary mismatch into a plausible loss. (One read-back: this is the scoring path.)
    bad = (lab != int(ignore_index)) & ((lab < 0) | (lab >= V))
    if bool(bad.any()):
        raise IndexError(f"cross_entropy: label {int(lab[bad][0])} outside the vocabulary ({V} columns)")
    nll = torch.empty((rows,), device=logits.device, dtype=torch.float32)
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    _lib.check(lib.vt_cross_entropy(_p(logits), rows, V, logits.stride(0), _p(lab), int(ignore_index), _p(nll), _p(loss), _stream()),
               "vt_cross_entropy", lib)
    return loss[0]


# ---- precise level 3: MX-FP4 images of the rounding remainders (include/vitron_hip.h "precise level 3") ---------------------------------
def mx4_aexp_bytes(M: int, K: int) -> int:
    return int(_lib.load_any().vt_mx4_aexp_bytes(M, K))


def mx4_quant_weights(w: torch.Tensor):
    """(W4 uint8 [N][K/2], wexp uint8 [N]) of a 16-bit weight matrix [N][K]."""
    lib, dt = _op16(w, "mx4_quant_weights.w")
    _chk(w, dt, "mx4_quant_weights.w")
    N, K = w.shape
    w4 = torch.empty((N, K // 2), device=w.device, dtype=torch.uint8)
    wexp = torch.empty((N,), device=w.device, dtype=torch.uint8)
    _lib.check(lib.vt_mx4_quant_weights(_p(w), K, N, K, _p(w4), _p(wexp), _stream()), "vt_mx4_quant_weights", lib)
    return w4, wexp


def mx4_quant_lo(lo: torch.Tensor):
    """(A4 uint8 [M][K/2], aexp uint8 [mx4_aexp_bytes(M, K)]) of a 16-bit remainder [M][K]."""
    lib, dt = _op16(lo, "mx4_quant_lo.lo")
    _chk(lo, dt, "mx4_quant_lo.lo")
    M, K = lo.shape
    a4 = torch.empty((M, K // 2), device=lo.device, dtype=torch.uint8)
    aexp = torch.zeros((mx4_aexp_bytes(M, K),), device=lo.device, dtype=torch.uint8)
    _lib.check(lib.vt_mx4_quant_lo(_p(lo), K, M, K, _p(a4), _p(aexp), _stream()), "vt_mx4_quant_lo", lib)
    return a4, aexp


def rmsnorm_mx(x: torch.Tensor, w: torch.Tensor, eps: float, dtype: torch.dtype, idx: Optional[torch.Tensor] = None):
    """(y op16 [rows][D], A4, aexp): RMSNorm with the level 3 operand out."""
    _chk(x, torch.float32, "rmsnorm_mx.x")
    _chk(w, torch.float32, "rmsnorm_mx.w")
    lib = _lib.load(operand=_lib.operand_of(dtype))
    rows = x.shape[0] if idx is None else idx.shape[0]
    D = x.shape[1]
    y = torch.empty((rows, D), device=x.device, dtype=dtype)
    a4 = torch.empty((rows, D // 2), device=x.device, dtype=torch.uint8)
    aexp = torch.zeros((mx4_aexp_bytes(rows, D),), device=x.device, dtype=torch.uint8)
    _lib.check(lib.vt_rmsnorm_mx(_p(x), _p(idx), _p(w), _p(y), _p(a4), _p(aexp), rows, D, eps, _stream()), "vt_rmsnorm_mx", lib)
    return y, a4, aexp


def gemm_mx(a: torch.Tensor, a4: torch.Tensor, aexp: torch.Tensor, w: torch.Tensor, w4: torch.Tensor, wexp: torch.Tensor,
            bias: Optional[torch.Tensor] = None, epi: int = EPI_BF16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = epi(a @ w^T + (a4 2^aexp) @ (w4 2^wexp)^T + bias) in one launch (vt_gemm_mx)."""
    lib, dt = _op16(a, "gemm_mx.a")
    _chk(a, dt, "gemm_mx.a")
    _chk(w, dt, "gemm_mx.w")
    for t, n in ((a4, "a4"), (aexp, "aexp"), (w4, "w4"), (wexp, "wexp")):
        _chk(t, torch.uint8, "gemm_mx." + n)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(a4.shape) != (M, K // 2) or tuple(w4.shape) != (N, K // 2) or wexp.numel() != N or \
            aexp.numel() < mx4_aexp_bytes(M, K):
        raise _lib.VitronHipError("gemm_mx: operand shapes do not match")
    if bias is not None:
        _chk(bias, torch.float32, "gemm_mx.bias")
    n_out = N // 2 if epi == EPI_SWIGLU_BF16 else N
    odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else dt
    if out is None:
        if epi == EPI_F32_RESID:
            raise _lib.VitronHipError("gemm_mx: EPI_F32_RESID needs `out` (the fp32 residual stream)")
        out = torch.empty((M, n_out), device=a.device, dtype=odt)
    _chk(out, odt, "gemm_mx.out")
    _lib.check(lib.vt_gemm_mx(_p(a), K, _p(a4), _p(aexp), _p(w), K, _p(w4), _p(wexp), _p(out), out.shape[1], _p(bias), M, N, K, epi,
                              _stream()), "vt_gemm_mx", lib)
    return out


def gemm_mx_swiglu(a, a4, aexp, w, w4, wexp):
    """(h op16 [M][N/2], h4 uint8 [M][N/4], hexp): level 3 gate/up -- the SwiGLU output and the MX-FP4 image of its rounding remainder."""
    lib, dt = _op16(a, "gemm_mx_swiglu.a")
    M, K = a.shape
    N = w.shape[0]
    h = torch.empty((M, N // 2), device=a.device, dtype=dt)
    h4 = torch.empty((M, N // 4), device=a.device, dtype=torch.uint8)
    hexp = torch.zeros((mx4_aexp_bytes(M, N // 2),), device=a.device, dtype=torch.uint8)
    _lib.check(lib.vt_gemm_mx_swiglu(_p(a), K, _p(a4), _p(aexp), _p(w), K, _p(w4), _p(wexp), _p(h), N // 2, _p(h4), _p(hexp), M, N, K, _stream()),
               "vt_gemm_mx_swiglu", lib)
    return h, h4, hexp


def gemm_mx_resid(a, a4, aexp, w, w4, wexp, out: torch.Tensor, partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32 [M][N]) += a @ w^T + (a4 2^aexp) @ (w4 2^wexp)^T; `partials` (fp32 scratch) lets a grid that spills over whole rounds run
    its trailing row blocks as K ranges (vt_gemm_mx_resid)."""
    lib, dt = _op16(a, "gemm_mx_resid.a")
    _chk(out, torch.float32, "gemm_mx_resid.out")
    M, K = a.shape
    N = w.shape[0]
    _lib.check(lib.vt_gemm_mx_resid(_p(a), K, _p(a4), _p(aexp), _p(w), K, _p(w4), _p(wexp), _p(out), N, M, N, K, _p(partials),
                                    0 if partials is None else partials.numel() * 4, _stream()), "vt_gemm_mx_resid", lib)
    return out


def flash_attn_mx(q, k_tiles, vt_tiles, tile_table, seq_desc, max_q_len: int, heads: int, scale: float):
    """Causal head_dim-128 attention with the level 3 operand out: (O op16 [rows][heads*128], O4, oexp). q: a [rows, ldq] view whose first
    heads*128 columns are the queries."""
    lib, dt = _op16(q, "flash_attn_mx.q")
    rows = q.shape[0]
    o = torch.empty((rows, heads * 128), device=q.device, dtype=dt)
    o4 = torch.empty((rows, heads * 64), device=q.device, dtype=torch.uint8)
    oexp = torch.zeros((mx4_aexp_bytes(rows, heads * 128),), device=q.device, dtype=torch.uint8)
    _lib.check(lib.vt_flash_attn_mx(_p(q), q.stride(0), _p(k_tiles), _p(vt_tiles), _p(tile_table), _p(seq_desc), seq_desc.shape[0], max_q_len,
                                    _p(o), heads * 128, _p(o4), _p(oexp), heads, scale, _stream()), "vt_flash_attn_mx", lib)
    return o, o4, oexp


def gemm_mx_gelu(a, a4, aexp, w, w4, wexp, bias: Optional[torch.Tensor] = None, quick: bool = False):
    """(h op16 [M][N], h4 uint8 [M][N/2], hexp): the towers' fc1 in precise level 1 -- gelu(a @ w^T + (a4..)(w4..)^T + bias) and the MX-FP4 image of
    its rounding remainder (vt_gemm_mx_gelu)."""
    lib, dt = _op16(a, "gemm_mx_gelu.a")
    M, K = a.shape
    N = w.shape[0]
    h = torch.empty((M, N), device=a.device, dtype=dt)
    h4 = torch.empty((M, N // 2), device=a.device, dtype=torch.uint8)
    hexp = torch.zeros((mx4_aexp_bytes(M, N),), device=a.device, dtype=torch.uint8)
    _lib.check(lib.vt_gemm_mx_gelu(_p(a), K, _p(a4), _p(aexp), _p(w), K, _p(w4), _p(wexp), _p(bias), _p(h), N, _p(h4), _p(hexp), M, N, K, int(quick),
                                   _stream()), "vt_gemm_mx_gelu", lib)
    return h, h4, hexp


def layernorm_mx(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, dtype: torch.dtype):
    """(y op16 [rows][D], A4, aexp): LayerNorm with the level 3 operand out (vt_layernorm_mx)."""
    _chk(x, torch.float32, "layernorm_mx.x")
    lib = _lib.load(operand=_lib.operand_of(dtype))
    rows, D = x.shape
    y = torch.empty((rows, D), device=x.device, dtype=dtype)
    a4 = torch.empty((rows, D // 2), device=x.device, dtype=torch.uint8)
    aexp = torch.zeros((mx4_aexp_bytes(rows, D),), device=x.device, dtype=torch.uint8)
    _lib.check(lib.vt_layernorm_mx(_p(x), _p(gamma), _p(beta), _p(y), _p(a4), _p(aexp), rows, D, eps, _stream()), "vt_layernorm_mx", lib)
    return y, a4, aexp


# ---- NF4 weight-only Linears (load_4bit; format: include/vitron_hip.h, vt_nf4_quant) -------------------------------------------
def nf4_quant(w: torch.Tensor, dtype=None):
    """(codes uint8 [N*K/2], absmax fp32 [N*K/64]) of a weight [N][K] in bitsandbytes' NF4 order: the weight is taken as fp16, blocks of
    64 consecutive elements, element 2j in the high nibble. `w` is fp32 or 16-bit; `dtype` (fp32 sources only) picks the library build
    (the codes do not depend on it)."""
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise _lib.VitronHipError("nf4_quant.w: expected a CUDA/HIP tensor (vitron_amd has no CPU path)")
    if w.dtype == torch.float32:
        lib, src = _lib.load(operand=_lib.operand_of(dtype or _lib.torch_dtype())), _lib.DTYPE_F32
    else:
        lib, _ = _op16(w, "nf4_quant.w")
        src = _lib.DTYPE_BF16   # VT_DTYPE_OP16: the library's own operand format
    _chk(w, w.dtype, "nf4_quant.w")
    N, K = w.shape
    if K % 64:
        raise _lib.VitronHipError(f"nf4_quant: K = {K} must be a multiple of 64")
    codes = torch.empty((N * K // 2,), device=w.device, dtype=torch.uint8)
    absmax = torch.empty((N * K // 64,), device=w.device, dtype=torch.float32)
    _lib.check(lib.vt_nf4_quant(_p(w), src, K, N, K, _p(codes), _p(absmax), _stream()), "vt_nf4_quant", lib)
    return codes, absmax


def _nf4_shape(codes: torch.Tensor, absmax: torch.Tensor, K: int, name: str) -> int:
    _chk(codes, torch.uint8, name + ".codes")
    _chk(absmax, torch.float32, name + ".absmax")
    if K <= 0 or K % 64 or (2 * codes.numel()) % K or codes.numel() * 2 // K * (K // 64) != absmax.numel():
        raise _lib.VitronHipError(f"{name}: {codes.numel()} code bytes / {absmax.numel()} scales do not describe a [N][{K}] NF4 matrix")
    return codes.numel() * 2 // K


def nf4_dequant(codes: torch.Tensor, absmax: torch.Tensor, K: int, dtype) -> torch.Tensor:
    """W [N][K] in `dtype` (the library's operand format) = op16(NF4[code] * absmax)."""
    lib = _lib.load(operand=_lib.operand_of(dtype))
    N = _nf4_shape(codes, absmax, K, "nf4_dequant")
    out = torch.empty((N, K), device=codes.device, dtype=_lib.torch_dtype(dtype))
    _lib.check(lib.vt_nf4_dequant(_p(codes), _p(absmax), N, K, _p(out), K, _stream()), "vt_nf4_dequant", lib)
    return out


def gemm_nf4(a: torch.Tensor, codes: torch.Tensor, absmax: torch.Tensor, epi: int = EPI_BF16, out: Optional[torch.Tensor] = None,
             norm_in: Optional[tuple] = None, norm_out: Optional[tuple] = None) -> torch.Tensor:
    """out = epi(a[M,K] @ dequant(W)[N,K]^T) on the 4-bit weight-streaming kernel, M <= 32 (EPI_BF16 / EPI_F32 / EPI_F32_RESID into `out` /
    EPI_SWIGLU_BF16). The decode step's folded RMSNorm (include/vitron_hip.h vt_gemm_nf4):
      norm_in  = (partials fp32 [M][in_n], inv_dim, eps): row m scaled by rsqrt(sum(partials[m]) * inv_dim + eps);
      norm_out = (w fp32 [N], xw op16 [M][N], partials fp32 [M][N/16]) with EPI_F32_RESID: xw = op16(x_new * w), partials = sums of x_new^2."""
    lib, dt = _op16(a, "gemm_nf4.a")
    _chk(a, dt, "gemm_nf4.a")
    M, K = a.shape
    N = _nf4_shape(codes, absmax, K, "gemm_nf4")
    n_out = N // 2 if epi == EPI_SWIGLU_BF16 else N
    odt = torch.float32 if epi in (EPI_F32, EPI_F32_RESID) else dt
    if out is None:
        if epi == EPI_F32_RESID:
            raise _lib.VitronHipError("gemm_nf4: EPI_F32_RESID needs `out` (the fp32 residual stream)")
        out = torch.empty((M, n_out), device=a.device, dtype=odt)
    _chk(out, odt, "gemm_nf4.out")
    if tuple(out.shape) != (M, n_out):
        raise _lib.VitronHipError(f"gemm_nf4: out is {tuple(out.shape)}, expected {(M, n_out)}")
    pin, in_n, inv_dim, eps = None, 0, 0.0, 0.0
    if norm_in is not None:
        pin, inv_dim, eps = norm_in
        _chk(pin, torch.float32, "gemm_nf4.norm_in")
        if pin.dim() != 2 or pin.shape[0] < M:
            raise _lib.VitronHipError("gemm_nf4: norm_in partials must be [M][in_n]")
        in_n = pin.shape[1]
    ow = oxw = opart = None
    if norm_out is not None:
        ow, oxw, opart = norm_out
        _chk(ow, torch.float32, "gemm_nf4.norm_out.w")
        _chk(oxw, dt, "gemm_nf4.norm_out.xw")
        _chk(opart, torch.float32, "gemm_nf4.norm_out.partials")
        if ow.numel() != N or tuple(oxw.shape) != (M, N) or opart.numel() < M * (N // 16):
            raise _lib.VitronHipError("gemm_nf4: norm_out shapes must be w [N], xw [M][N], partials [M][N/16]")
    _lib.check(lib.vt_gemm_nf4(_p(a), K, _p(codes), _p(absmax), _p(out), n_out, M, N, K, epi, _p(pin), in_n, float(inv_dim), float(eps),
                               _p(ow), _p(oxw), N, _p(opart), _stream()), "vt_gemm_nf4", lib)
    return out
