"""Python front-end of the C ABI for tests and benchmarks.

PyTorch is plumbing here: it owns device buffers (int64 tensors holding the raw
u64 words) and the current HIP stream, and provides torch.distributed for
multi-GPU runs.  Every operation is a call into libhehub_amd.so; nothing is
computed by torch or numpy.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import capi


class HpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[hp_status {code}] {msg}")
        self.code = code
        self.msg = msg


class InvalidArgument(HpError, ValueError):
    """The reference throws std::invalid_argument for the same input."""


def _u64arr(v: Sequence[int]):
    return (capi.u64 * len(v))(*[int(x) for x in v])


class Engine:
    """One engine context on one GPU (include/hehub_amd.h: hp_ctx)."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        import torch  # noqa: F401  (loads the HIP runtime the library binds to)

        self.torch = torch
        if not torch.cuda.is_available():
            raise capi.EngineMissing("no HIP device visible: the engine needs an MI355X (no CPU fallback)")
        self.lib = capi.load()
        self.device = device
        torch.cuda.set_device(device)
        h = capi.P()
        rc = self.lib.hp_ctx_create(device, C.byref(h))
        if rc != capi.HP_OK:
            raise HpError(rc, "hp_ctx_create failed")
        self.h = h
        if use_torch_stream:
            self.use_stream(torch.cuda.current_stream(device))

    def fork(self) -> "Engine":
        """A second lane on the same GPU (hp_ctx_fork): its own stream and scratch workspace, the family's tables and lock; calls on it
        overlap on the device with calls on this one.  Order them with wait_for where one reads what the other wrote.
        A lane's stream is not torch's: torch's caching allocator recycles a freed tensor's block at once, so keep every tensor a lane's
        calls touch referenced until that lane has been synchronised (sync / wait_for), and wait for copies torch makes on its own stream
        before a lane reads them."""
        e = object.__new__(Engine)
        e.torch, e.lib, e.device = self.torch, self.lib, self.device
        h = capi.P()
        self._chk(self.lib.hp_ctx_fork(self.h, C.byref(h)))
        e.h = h
        return e

    def wait_for(self, other: "Engine"):
        """everything enqueued on this context from now on runs after everything `other` has enqueued so far (device-side event)"""
        self._chk(self.lib.hp_ctx_wait_for(self.h, other.h))

    def gather_rows(self, rows, words: int, out):
        """rows: device tensors (each `words` int64 words, anywhere) -> out[len(rows)][words] by one kernel per 64 rows"""
        ptrs = (capi.P * len(rows))(*[r.data_ptr() for r in rows])
        self._chk(self.lib.hp_dev_gather_rows(self.h, len(rows), words, ptrs, self._ptr(out)))
        return out

    def scatter_rows(self, packed, words: int, rows):
        ptrs = (capi.P * len(rows))(*[r.data_ptr() for r in rows])
        self._chk(self.lib.hp_dev_scatter_rows(self.h, len(rows), words, self._ptr(packed), ptrs))

    def close(self):
        if getattr(self, "h", None):
            self.lib.hp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -----------------------------------------------------------
    def _chk(self, rc: int):
        if rc == capi.HP_OK:
            return
        msg = self.lib.hp_last_error(self.h).decode()
        if rc == capi.HP_EINVAL:
            raise InvalidArgument(rc, msg)
        raise HpError(rc, msg)

    def use_stream(self, stream):
        self._chk(self.lib.hp_ctx_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def sync(self):
        self._chk(self.lib.hp_sync(self.h))

    def workspace_bytes(self) -> int:
        return int(self.lib.hp_ctx_workspace_bytes(self.h))

    def release_workspace(self):
        self._chk(self.lib.hp_ctx_release_workspace(self.h))

    def force_generic(self, on: bool):
        self._chk(self.lib.hp_ctx_set_force_generic(self.h, int(on)))

    def set_parity_level(self, level: str):
        """"B" (default): raw words identical to hehub's.  "A": the scheme-level pipelines return canonical residues through
        the FP64 transforms (include/hehub_amd.h: hp_ctx_set_parity_level); the NTT / mod-arith primitives are never affected."""
        self._chk(self.lib.hp_ctx_set_parity_level(self.h, {"B": 0, "A": 1}[level.upper()]))

    def parity_level(self) -> str:
        return "BA"[self.lib.hp_ctx_get_parity_level(self.h)]

    def set_error_sampler(self, kind: int):
        """the error distribution of the seeded key and ciphertext calls: 3 (centred binomial, the default) or 4 (discrete Gaussian of
        sigma 3.2); include/hehub_amd.h: hp_ctx_set_error_sampler.  A fork inherits it."""
        self._chk(self.lib.hp_ctx_set_error_sampler(self.h, kind))

    def get_error_sampler(self) -> int:
        return int(self.lib.hp_ctx_get_error_sampler(self.h))

    def to_device(self, a: np.ndarray):
        assert a.dtype == np.uint64
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(f"cuda:{self.device}")

    @staticmethod
    def to_host(t) -> np.ndarray:
        return t.detach().cpu().numpy().view(np.uint64)

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.int64, device=f"cuda:{self.device}")

    @staticmethod
    def _ptr(t):
        assert t.is_contiguous() and t.element_size() == 8
        return C.c_void_p(t.data_ptr())

    # -- profiling ---------------------------------------------------------
    def prof_begin(self, family: str):
        self._chk(self.lib.hp_prof_begin(self.h, family.encode()))

    def prof_end(self):
        n = capi.szt(0)
        ms = C.c_double(0)
        self._chk(self.lib.hp_prof_end(self.h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def prof_end_families(self):
        """after prof_begin("*"): {family: (launches, total ms)} of every bracketed launch, in order of first appearance"""
        cap = 32
        names = (C.c_char_p * cap)()
        launches = (capi.szt * cap)()
        ms = (C.c_double * cap)()
        count = capi.szt(0)
        self._chk(self.lib.hp_prof_end_families(self.h, cap, names, launches, ms, C.byref(count)))
        return {names[i].decode(): (int(launches[i]), float(ms[i])) for i in range(int(count.value))}

    # -- drop-in host calls (numpy in, numpy out) ----------------------------
    def host_ntt(self, logn: int, q: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x.copy())
        self._chk(self.lib.hp_ntt_negacyclic_inplace_lazy(self.h, logn, q, x.ctypes.data_as(capi.P)))
        return x

    def host_intt(self, logn: int, q: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x.copy())
        self._chk(self.lib.hp_intt_negacyclic_inplace_lazy(self.h, logn, q, x.ctypes.data_as(capi.P)))
        return x

    def cache_ntt_factors_strict(self, logn: int, moduli):
        self._chk(self.lib.hp_cache_ntt_factors_strict(self.h, logn, _u64arr(moduli), len(moduli)))

    def _host_inplace(self, fn, q, v):
        v = np.ascontiguousarray(v.copy())
        self._chk(fn(self.h, q, v.size, v.ctypes.data_as(capi.P)))
        return v

    def host_barrett_lazy(self, q, v):
        return self._host_inplace(self.lib.hp_batched_barrett_lazy, q, v)

    def host_barrett(self, q, v):
        return self._host_inplace(self.lib.hp_batched_barrett, q, v)

    def host_reduce_strict(self, q, v):
        return self._host_inplace(self.lib.hp_batched_reduce_strict, q, v)

    def host_mul_hybrid_lazy(self, q, a, b):
        out = np.empty_like(a)
        self._chk(self.lib.hp_batched_mul_mod_hybrid_lazy(self.h, q, a.size, a.ctypes.data_as(capi.P),
                                                          b.ctypes.data_as(capi.P), out.ctypes.data_as(capi.P)))
        return out

    def host_mul_barrett_lazy(self, q, a, b):
        out = np.empty_like(a)
        self._chk(self.lib.hp_batched_mul_mod_barrett_lazy(self.h, q, a.size, a.ctypes.data_as(capi.P),
                                                           b.ctypes.data_as(capi.P), out.ctypes.data_as(capi.P)))
        return out

    def host_montgomery_128_lazy(self, q, in128):
        in128 = np.ascontiguousarray(in128)
        out = np.empty(in128.shape[0], dtype=np.uint64)
        self._chk(self.lib.hp_batched_montgomery_128_lazy(self.h, q, out.size, in128.ctypes.data_as(capi.P),
                                                          out.ctypes.data_as(capi.P)))
        return out

    # -- device batches: tensors [batch, L, N] of int64 (raw u64 words) --------
    def ntt_(self, moduli, x):
        B, L, n = x.shape
        self._chk(self.lib.hp_dev_ntt(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(x)))
        return x

    def intt_(self, moduli, x, strict: bool = False):
        B, L, n = x.shape
        self._chk(self.lib.hp_dev_intt(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(x), int(strict)))
        return x

    def ntt_residues_(self, moduli, x):
        """forward transforms in place to CANONICAL residues (hp_dev_ntt_residues: the FP64 kernels; == oracle ntt words mod q)"""
        B, L, n = x.shape
        self._chk(self.lib.hp_dev_ntt_residues(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(x)))
        return x

    def intt_residues_(self, moduli, x):
        """inverse transforms in place, strict (hp_dev_intt_residues: the words of intt_negacyclic_inplace)"""
        B, L, n = x.shape
        self._chk(self.lib.hp_dev_intt_residues(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(x)))
        return x

    def _binary(self, fn, moduli, a, b, out=None):
        B, L, n = a.shape
        out = self.empty(a.shape) if out is None else out
        self._chk(fn(self.h, n, L, _u64arr(moduli), B, self._ptr(a), self._ptr(b), self._ptr(out)))
        return out

    def poly_add(self, moduli, a, b, out=None):
        return self._binary(self.lib.hp_dev_poly_add, moduli, a, b, out)

    def poly_fold_rows(self, moduli, chains, negate, out=None):
        """chains[p] = the term polynomials (device tensors [L][n], anywhere) of polynomial p; out[p] = ((x0 op1 x1) op2 x2) ... with
        op_j = -= where negate[j] (include/hehub_amd.h: hp_dev_poly_fold_rows): the words of the chain of += / -= calls"""
        polys, terms = len(chains), len(chains[0])
        L, n = chains[0][0].shape
        if out is None:
            out = self.empty((polys, L, n))
        ptrs = (capi.P * (polys * terms))(*[t.data_ptr() for c in chains for t in c])
        neg = (C.c_uint8 * terms)(*[1 if x else 0 for x in negate])
        self._chk(self.lib.hp_dev_poly_fold_rows(self.h, n, L, _u64arr(moduli), polys, terms, neg, ptrs, self._ptr(out)))
        return out

    def poly_sub(self, moduli, a, b, out=None):
        return self._binary(self.lib.hp_dev_poly_sub, moduli, a, b, out)

    def poly_mul(self, moduli, a, b, out=None):
        return self._binary(self.lib.hp_dev_poly_mul, moduli, a, b, out)

    def poly_scalar_mul(self, moduli, a, scalars, out=None):
        B, L, n = a.shape
        if isinstance(scalars, int):
            scalars = [scalars] * L
        if len(scalars) != L:
            raise InvalidArgument(capi.HP_EINVAL, "Numbers of RNS component mismatch.")
        out = self.empty(a.shape) if out is None else out
        self._chk(self.lib.hp_dev_poly_scalar_mul(self.h, n, L, _u64arr(moduli), B, _u64arr(scalars), self._ptr(a),
                                                  self._ptr(out)))
        return out

    def poly_reduce_strict_(self, moduli, x):
        B, L, n = x.shape
        self._chk(self.lib.hp_dev_poly_reduce_strict(self.h, n, L, _u64arr(moduli), B, self._ptr(x)))
        return x

    def copy(self, src, out=None):
        """deep copy of device words (hp_dev_copy)"""
        out = self.empty(src.shape) if out is None else out
        # the kernel writes src.numel() words at out's address: a short, strided or foreign `out` would be written past its end
        for t in (src, out):
            if t.element_size() != 8 or not t.is_contiguous() or t.device.type != "cuda" or t.device.index != self.device:
                raise InvalidArgument(capi.HP_EINVAL, "copy: contiguous 8-byte tensors on the engine's device")
        if out.numel() != src.numel():
            raise InvalidArgument(capi.HP_EINVAL, f"copy: out holds {out.numel()} words, src {src.numel()}")
        self._chk(self.lib.hp_dev_copy(self.h, src.numel(), self._ptr(src), self._ptr(out)))
        return out

    def poly_involution(self, a):
        B, L, n = a.shape
        out = self.empty(a.shape)
        self._chk(self.lib.hp_dev_poly_involution(self.h, n.bit_length() - 1, L, B, self._ptr(a), self._ptr(out)))
        return out

    def poly_cycle(self, a, step: int):
        B, L, n = a.shape
        out = self.empty(a.shape)
        self._chk(self.lib.hp_dev_poly_cycle(self.h, n.bit_length() - 1, L, B, step, self._ptr(a), self._ptr(out)))
        return out

    # -- scheme level: ciphertext batches [batch, 2|3, L, N] -------------------
    def mult_low_level(self, moduli, ct1, ct2):
        B, two, L, n = ct1.shape
        out = self.empty((B, 3, L, n))
        self._chk(self.lib.hp_dev_mult_low_level(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(ct1),
                                                 self._ptr(ct2), self._ptr(out)))
        return out

    def ext_prod(self, moduli_ext, pt, key):
        B, L, n = pt.shape
        out = self.empty((B, 2, L + 1, n))
        self._chk(self.lib.hp_dev_ext_prod_montgomery(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), B,
                                                      self._ptr(pt), self._ptr(key), self._ptr(out)))
        return out

    def ckks_rescale(self, moduli, ct):
        B, two, L, n = ct.shape
        out = self.empty((B, 2, max(L - 1, 1), n))
        self._chk(self.lib.hp_dev_ckks_rescale(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(ct),
                                               self._ptr(out)))
        return out

    def bgv_mod_switch(self, moduli, t, ct):
        B, two, L, n = ct.shape
        out = self.empty((B, 2, max(L - 1, 1), n))
        self._chk(self.lib.hp_dev_bgv_mod_switch(self.h, n.bit_length() - 1, L, _u64arr(moduli), t, B, self._ptr(ct),
                                                 self._ptr(out)))
        return out

    def ckks_relinearize(self, moduli_ext, quad, key):
        B, three, L, n = quad.shape
        out = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_ckks_relinearize(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), B,
                                                   self._ptr(quad), self._ptr(key), self._ptr(out)))
        return out

    def bgv_relinearize(self, moduli_ext, quad, key, inner_t: int = 1):
        B, three, L, n = quad.shape
        out = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_bgv_relinearize(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), inner_t, B,
                                                  self._ptr(quad), self._ptr(key), self._ptr(out)))
        return out

    def ckks_rotate(self, moduli_ext, ct, key, step: int):
        B, two, L, n = ct.shape
        out = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_ckks_rotate(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), B, step, self._ptr(ct),
                                              self._ptr(key), self._ptr(out)))
        return out

    def ckks_conjugate(self, moduli_ext, ct, key):
        B, two, L, n = ct.shape
        out = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_ckks_conjugate(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), B, self._ptr(ct),
                                                 self._ptr(key), self._ptr(out)))
        return out

    # -- extensions beyond the reference (include/hehub_amd.h) ----------------
    def ckks_mult_at(self, moduli_ext, key_L0: int, ct1, ct2, key):
        """ckks::mult + rescale at level L = ct limbs with a key generated for key_L0 >= L ciphertext moduli."""
        B, _, L, n = ct1.shape
        out = self.empty((B, 2, L - 1, n))
        self._chk(self.lib.hp_dev_ckks_mult_relin_rescale_at(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B,
                                                             self._ptr(ct1), self._ptr(ct2), self._ptr(key), self._ptr(out)))
        return out

    def ckks_rotate_at(self, moduli_ext, key_L0: int, ct, key, step: int):
        B, _, L, n = ct.shape
        out = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_ckks_rotate_at(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B, step,
                                                 self._ptr(ct), self._ptr(key), self._ptr(out)))
        return out

    def ckks_mult_rows(self, moduli_ext, key_L0: int, pairs, key):
        """ckks::mult + rescale with the operands by address: pairs[b] = (a0, a1, b0, b1), device tensors [L][n] anywhere"""
        B = len(pairs)
        L, n = pairs[0][0].shape
        out = self.empty((B, 2, L - 1, n))
        pp = (capi.P * (4 * B))(*[p.data_ptr() for quad in pairs for p in quad])
        self._chk(self.lib.hp_dev_ckks_mult_relin_rescale_rows(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B, pp,
                                                               self._ptr(key), self._ptr(out)))
        return out

    def bgv_mult_rows(self, moduli_ext, t: int, pairs, key):
        B = len(pairs)
        L, n = pairs[0][0].shape
        out = self.empty((B, 2, L - 1, n))
        pp = (capi.P * (4 * B))(*[p.data_ptr() for quad in pairs for p in quad])
        self._chk(self.lib.hp_dev_bgv_mult_relin_modswitch_rows(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), t, B, pp,
                                                                self._ptr(key), self._ptr(out)))
        return out

    def ckks_rotate_many(self, moduli_ext, key_L0: int, ct, keys, steps, conj=None):
        """ciphertext b rotated by steps[b] (conjugated where conj[b]) and switched with ITS OWN key keys[b] (device tensors)."""
        B, _, L, n = ct.shape
        assert len(keys) == B and len(steps) == B
        out = self.empty((B, 2, L, n))
        kp = (capi.P * B)(*[k.data_ptr() for k in keys])
        st = (C.c_size_t * B)(*[int(s) for s in steps])
        cj = (C.c_ubyte * B)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._chk(self.lib.hp_dev_ckks_rotate_many(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B, st, cj,
                                                   self._ptr(ct), kp, self._ptr(out)))
        return out

    def ckks_rotate_many_rows(self, moduli_ext, key_L0: int, polys, keys, steps, conj=None):
        """the same with the polynomials of ciphertext b anywhere on the device: polys[b] = (poly0, poly1), tensors [L][n]"""
        B = len(polys)
        L, n = polys[0][0].shape
        assert len(keys) == B and len(steps) == B
        out = self.empty((B, 2, L, n))
        pp = (capi.P * (2 * B))(*[p.data_ptr() for pair in polys for p in pair])
        kp = (capi.P * B)(*[k.data_ptr() for k in keys])
        st = (C.c_size_t * B)(*[int(s) for s in steps])
        cj = (C.c_ubyte * B)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._chk(self.lib.hp_dev_ckks_rotate_many_rows(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B, st, cj, pp, kp,
                                                        self._ptr(out)))
        return out

    def ext_prod_at(self, moduli_ext, key_L0: int, pt, key):
        B, L, n = pt.shape
        out = self.empty((B, 2, L + 1, n))
        self._chk(self.lib.hp_dev_ext_prod_montgomery_at(self.h, n.bit_length() - 1, L, key_L0, _u64arr(moduli_ext), B,
                                                         self._ptr(pt), self._ptr(key), self._ptr(out)))
        return out

    def rns_base_many_to_many(self, old_moduli, new_moduli, x):
        B, L, n = x.shape
        out = self.empty((B, len(new_moduli), n))
        self._chk(self.lib.hp_dev_rns_base_many_to_many(self.h, n, L, _u64arr(old_moduli), len(new_moduli), _u64arr(new_moduli), B,
                                                        self._ptr(x), self._ptr(out)))
        return out

    def _hks(self, name, key_L0, logn, L, *rest):
        """a hybrid call over keys: the plain entry point, or with key_L0 (the ciphertext moduli the keys -- and diagonals -- were
        generated for, >= L: one top-level key set serves every level) its _at form, which takes key_L0 after L"""
        if key_L0 is None:
            return self._chk(getattr(self.lib, name)(self.h, logn, L, *rest))
        return self._chk(getattr(self.lib, name + "_at")(self.h, logn, L, int(key_L0), *rest))

    def hks_switch(self, moduli_ext, k: int, alpha: int, pt, key, key_L0=None):
        """hybrid key switch (extension): pt [B][L][n] NTT form, key [dnum][2][L+k][n] -> [B][2][L][n].  key_L0 (here and in every
        hybrid method over keys): the keys are [ceil(key_L0/alpha)][2][key_L0+k][n], generated for key_L0 >= L moduli; moduli_ext stays
        the level's chain."""
        B, L, n = pt.shape
        out = self.empty((B, 2, L, n))
        self._hks("hp_dev_hks_switch", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, self._ptr(pt),
                  self._ptr(key), self._ptr(out))
        return out

    def ckks_rotate_hks(self, moduli_ext, k: int, alpha: int, ct, key, step: int, key_L0=None):
        B, _, L, n = ct.shape
        out = self.empty((B, 2, L, n))
        self._hks("hp_dev_ckks_rotate_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, step,
                  self._ptr(ct), self._ptr(key), self._ptr(out))
        return out

    def ckks_conjugate_hks(self, moduli_ext, k: int, alpha: int, ct, key, key_L0=None):
        B, _, L, n = ct.shape
        out = self.empty((B, 2, L, n))
        self._hks("hp_dev_ckks_conjugate_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B,
                  self._ptr(ct), self._ptr(key), self._ptr(out))
        return out

    def ckks_rotate_hoisted_hks(self, moduli_ext, k: int, alpha: int, ct, keys, steps, conj=None, key_L0=None):
        """every ciphertext of ct [B][2][L][n] rotated by steps[r] (conjugated where conj[r]) under ITS hybrid key keys[r] (device
        tensors), all rotations sharing one digit decomposition of c1 -> [B][R][2][L][n]."""
        B, _, L, n = ct.shape
        R = len(keys)
        assert len(steps) == R and (conj is None or len(conj) == R)
        out = self.empty((B, R, 2, L, n))
        kp = (capi.P * R)(*[key.data_ptr() for key in keys])
        st = (C.c_size_t * R)(*[int(s) for s in steps])
        cj = (C.c_ubyte * R)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._hks("hp_dev_ckks_rotate_hoisted_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, R, st, cj,
                  self._ptr(ct), kp, self._ptr(out))
        return out

    def ckks_lintrans_hks(self, moduli_ext, k: int, alpha: int, ct, keys, steps, diags, conj=None, key_L0=None):
        """sum_r diags[r] * rot_r(ct) for ct [B][2][L][n] with one hybrid key per rotation, the weighted sum formed before ONE ModDown
        -> [B][2][L][n].  diags[r]: device tensor [L+k][n], NTT form over the extended chain, plain lazy words; None: the constant 1.
        With key_L0 the diagonals are [key_L0+k][n] like the keys' digits: encoded once over the top chain."""
        B, _, L, n = ct.shape
        R = len(keys)
        assert len(steps) == R and len(diags) == R and (conj is None or len(conj) == R)
        out = self.empty((B, 2, L, n))
        kp = (capi.P * R)(*[key.data_ptr() for key in keys])
        dp = (capi.P * R)(*[None if d is None else d.data_ptr() for d in diags])
        st = (C.c_size_t * R)(*[int(s) for s in steps])
        cj = (C.c_ubyte * R)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._hks("hp_dev_ckks_lintrans_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, R, st, cj,
                  self._ptr(ct), kp, dp, self._ptr(out))
        return out

    def ckks_lintrans_bsgs_hks(self, moduli_ext, k: int, alpha: int, ct, baby_keys, baby_steps, giant_keys, giant_steps, diags,
                               baby_conj=None, giant_conj=None, key_L0=None):
        """sum_g rot_g( sum_i diags[g][i] * rot_i(ct) ) for ct [B][2][L][n]: len(baby_keys) + len(giant_keys) hybrid keys for their
        product of diagonals -> [B][2][L][n].  diags[g][i]: device tensor [L+k][n], NTT form over the extended chain, plain lazy words,
        NOT rotated by the call (pass rot_g^-1 of the matrix's diagonal g + i); None: the term is ABSENT (in ckks_lintrans_hks None is
        the constant 1).  A key may be None where the step is 0 and the entry no conjugation: the identity, no key switch.
        With key_L0 the diagonals are [key_L0+k][n] like the keys' digits."""
        B, _, L, n = ct.shape
        nb, ng = len(baby_keys), len(giant_keys)
        assert len(baby_steps) == nb and len(giant_steps) == ng and len(diags) == ng and all(len(row) == nb for row in diags)
        assert (baby_conj is None or len(baby_conj) == nb) and (giant_conj is None or len(giant_conj) == ng)
        out = self.empty((B, 2, L, n))

        def table(keys, steps, conj):
            cnt = len(keys)
            return ((C.c_size_t * cnt)(*[int(s) for s in steps]),
                    (C.c_ubyte * cnt)(*[1 if c else 0 for c in conj]) if conj is not None else None,
                    (capi.P * cnt)(*[None if key is None else key.data_ptr() for key in keys]))

        bs, bc, bk = table(baby_keys, baby_steps, baby_conj)
        gs, gc, gk = table(giant_keys, giant_steps, giant_conj)
        dp = (capi.P * (ng * nb))(*[None if d is None else d.data_ptr() for row in diags for d in row])
        self._hks("hp_dev_ckks_lintrans_bsgs_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, nb, bs, bc, bk,
                  ng, gs, gc, gk, dp, self._ptr(ct), self._ptr(out))
        return out

    def ckks_mult_hks(self, moduli_ext, k: int, alpha: int, ct1, ct2, key, out=None, key_L0=None):
        B, _, L, n = ct1.shape
        out = self.empty((B, 2, L - 1, n)) if out is None else out
        self._hks("hp_dev_ckks_mult_relin_rescale_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B,
                  self._ptr(ct1), self._ptr(ct2), self._ptr(key), self._ptr(out))
        return out

    @staticmethod
    def _terms(a_list, b_list):
        """two lists of ciphertext batches [B][2][L][n] (device tensors) as ctypes arrays of addresses"""
        T = len(a_list)
        assert len(b_list) == T and T > 0
        shape = a_list[0].shape
        assert all(t.shape == shape and t.is_contiguous() and t.element_size() == 8 for t in list(a_list) + list(b_list))
        return T, (capi.P * T)(*[t.data_ptr() for t in a_list]), (capi.P * T)(*[t.data_ptr() for t in b_list])

    def ckks_tensor_sum(self, moduli, a_list, b_list, out=None):
        """sum_t a_list[t] (x) b_list[t] for ciphertext batches [B][2][L][n] (device tensors anywhere; words below 2q) ->
        the quadratic ciphertexts [B][3][L][n] in mult_low_level's layout, by one streaming kernel.  a_list may be b_list (squares)."""
        B, _, L, n = a_list[0].shape
        T, ap, bp = self._terms(a_list, b_list)
        out = self.empty((B, 3, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_ckks_tensor_sum(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, T, ap, bp, self._ptr(out)))
        return out

    def ckks_relin_rescale_hks(self, moduli_ext, k: int, alpha: int, quad, key, out=None, key_L0=None):
        """quad [B][3][L][n] (mult_low_level's or ckks_tensor_sum's) -> hybrid relinearisation + rescale, [B][2][L-1][n]"""
        B, _, L, n = quad.shape
        out = self.empty((B, 2, L - 1, n)) if out is None else out
        self._hks("hp_dev_ckks_relin_rescale_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B,
                  self._ptr(quad), self._ptr(key), self._ptr(out))
        return out

    def ckks_dot_hks(self, moduli_ext, k: int, alpha: int, a_list, b_list, key, out=None, key_L0=None):
        """rescale(relin(sum_t a_list[t] (x) b_list[t])) with ONE hybrid key switch whatever the number of terms -> [B][2][L-1][n]"""
        B, _, L, n = a_list[0].shape
        T, ap, bp = self._terms(a_list, b_list)
        out = self.empty((B, 2, L - 1, n)) if out is None else out
        self._hks("hp_dev_ckks_dot_relin_rescale_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), B, T, ap, bp,
                  self._ptr(key), self._ptr(out))
        return out

    def ckks_lincomb(self, moduli, cts, coefs=None, cst=None, out=None):
        """sum_j coefs[j] * cts[j] + cst over the L = len(moduli) first limbs of ciphertext batches [B][2][L_j][n], L_j >= L (device
        tensors anywhere; words below 2q) -> [B][2][L][n], canonical words, by one streaming kernel.  coefs[j]: the L residues of an
        integer constant (None: 1); cst: L residues added to every position of polynomial 0 (None: 0)."""
        T, L = len(cts), len(moduli)
        B, _, _, n = cts[0].shape
        assert T > 0 and all(t.shape[0] == B and t.shape[1] == 2 and t.shape[3] == n and t.is_contiguous() and t.element_size() == 8 for t in cts)
        assert coefs is None or len(coefs) == T
        out = self.empty((B, 2, L, n)) if out is None else out
        cp = (capi.P * T)(*[t.data_ptr() for t in cts])
        limbs = (C.c_size_t * T)(*[int(t.shape[2]) for t in cts])
        keep = [None if coefs is None or c is None else _u64arr(c) for c in (coefs if coefs is not None else [None] * T)]
        kp = None if coefs is None else (capi.P * T)(*[None if c is None else C.addressof(c) for c in keep])
        self._chk(self.lib.hp_dev_ckks_lincomb(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, T, cp, limbs, kp,
                                               None if cst is None else _u64arr(cst), self._ptr(out)))
        return out

    def ckks_poly_eval_hks(self, moduli_ext, k: int, alpha: int, ct, key, plan, key_L0=None):
        """a plan of hehub_amd.polyeval (build_plan: a polynomial in the power or the Chebyshev basis) evaluated on the ciphertext
        batch ct [B][2][L][n] with ONE relinearisation key (hks_keygen's for s * s, generated for key_L0 >= L moduli; None: L)
        -> [B][2][plan.out_limbs][n]"""
        B, _, L, n = ct.shape
        assert len(moduli_ext) == L + k and plan.in_limbs == L
        steps, keep = plan.marshal()
        out = self.empty((B, 2, plan.out_limbs, n))
        self._chk(self.lib.hp_dev_ckks_eval_plan_hks(self.h, n.bit_length() - 1, L, L if key_L0 is None else int(key_L0), k, alpha,
                                                     _u64arr(moduli_ext), B, len(plan.steps), steps, plan.final_drops, self._ptr(ct),
                                                     self._ptr(key), self._ptr(out)))
        del keep
        return out

    # -- BGV over the hybrid key switch: t = the plain modulus; keys are hks_keygen's / hks_keygen_rot's for error rows t * e ----------
    def bgv_hks_switch(self, moduli_ext, t: int, k: int, alpha: int, pt, key, out=None, key_L0=None):
        """hks_switch with the plain-modulus ModDown: pt [B][L][n] -> [B][2][L][n], out0 + out1 s_to = pt s_from + t * (small)"""
        B, L, n = pt.shape
        out = self.empty((B, 2, L, n)) if out is None else out
        self._hks("hp_dev_bgv_hks_switch", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), t, B, self._ptr(pt),
                  self._ptr(key), self._ptr(out))
        return out

    def bgv_rotate_hoisted_hks(self, moduli_ext, t: int, k: int, alpha: int, ct, keys, steps, conj=None, out=None, key_L0=None):
        """ckks_rotate_hoisted_hks for BGV ciphertexts: the cycle by steps[r] rotates the two slot rows, conj[r] swaps them
        -> [B][R][2][L][n].  One rotation is a list of one."""
        B, _, L, n = ct.shape
        R = len(keys)
        assert len(steps) == R and (conj is None or len(conj) == R)
        out = self.empty((B, R, 2, L, n)) if out is None else out
        kp = (capi.P * R)(*[None if key is None else key.data_ptr() for key in keys])
        st = (C.c_size_t * R)(*[int(s) for s in steps])
        cj = (C.c_ubyte * R)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._hks("hp_dev_bgv_rotate_hoisted_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), t, B, R, st, cj,
                  self._ptr(ct), kp, self._ptr(out))
        return out

    def bgv_relin_modswitch_hks(self, moduli_ext, t: int, k: int, alpha: int, quad, key, out=None, key_L0=None):
        """quad [B][3][L][n] (mult_low_level's or ckks_tensor_sum's) -> hybrid relinearisation + BGV mod switch, [B][2][L-1][n]"""
        B, _, L, n = quad.shape
        out = self.empty((B, 2, max(L - 1, 1), n)) if out is None else out
        self._hks("hp_dev_bgv_relin_modswitch_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), t, B,
                  self._ptr(quad), self._ptr(key), self._ptr(out))
        return out

    def bgv_mult_hks(self, moduli_ext, t: int, k: int, alpha: int, ct1, ct2, key, out=None, key_L0=None):
        """bgv::mult with a hybrid relinearisation key + mod switch by the last ciphertext modulus -> [B][2][L-1][n]"""
        B, _, L, n = ct1.shape
        out = self.empty((B, 2, max(L - 1, 1), n)) if out is None else out
        self._hks("hp_dev_bgv_mult_relin_modswitch_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), t, B,
                  self._ptr(ct1), self._ptr(ct2), self._ptr(key), self._ptr(out))
        return out

    # -- BFV: moduli_qb = q_0..q_{L-1}, b_0..b_{M-1} (the auxiliary base), t = the plain modulus; canonical words out --------------------
    def bfv_lift(self, moduli_qb, L: int, x, out=None):
        """x [B][L][n] NTT form over Q -> [B][L+M][n]: the Q rows carried over, the B rows of the exact centred integer behind x"""
        B, Lx, n = x.shape
        assert Lx == L
        E = len(moduli_qb)
        out = self.empty((B, E, n)) if out is None else out
        self._chk(self.lib.hp_dev_bfv_lift(self.h, n.bit_length() - 1, L, E - L, _u64arr(moduli_qb), B, self._ptr(x), self._ptr(out)))
        return out

    def bfv_scale_round(self, moduli_qb, L: int, t: int, x, out=None):
        """x [B][L+M][n] NTT form over Q B -> [B][L][n]: floor((t x + h) / Q), h = (Q - 1) / 2, of every coefficient"""
        B, E, n = x.shape
        assert E == len(moduli_qb)
        out = self.empty((B, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_bfv_scale_round(self.h, n.bit_length() - 1, L, E - L, _u64arr(moduli_qb), t, B, self._ptr(x), self._ptr(out)))
        return out

    def bfv_mult_low_level(self, moduli_qb, t: int, ct1, ct2, out=None):
        """the scale-invariant product of BFV ciphertexts [B][2][L][n] -> the quadratic ciphertext [B][3][L][n]"""
        B, _, L, n = ct1.shape
        out = self.empty((B, 3, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_bfv_mult_low_level(self.h, n.bit_length() - 1, L, len(moduli_qb) - L, _u64arr(moduli_qb), t, B,
                                                     self._ptr(ct1), self._ptr(ct2), self._ptr(out)))
        return out

    def bfv_mult_hks(self, moduli_ext, aux_moduli, t: int, k: int, alpha: int, ct1, ct2, key, out=None, key_L0=None):
        """bfv_mult_low_level + relinearisation with a hybrid key (hks_keygen's for s_from = s * s, plain error rows) -> [B][2][L][n]"""
        B, _, L, n = ct1.shape
        out = self.empty((B, 2, L, n)) if out is None else out
        self._hks("hp_dev_bfv_mult_relin_hks", key_L0, n.bit_length() - 1, L, k, alpha, _u64arr(moduli_ext), len(aux_moduli),
                  _u64arr(aux_moduli), t, B, self._ptr(ct1), self._ptr(ct2), self._ptr(key), self._ptr(out))
        return out

    def bfv_decrypt_round(self, moduli, t: int, x, out=None):
        """x [B][L][n] strict coefficient rows of c0 + c1 s (rlwe_decrypt_core's) -> the plaintext [B][n], words below t"""
        B, L, n = x.shape
        out = self.empty((B, n)) if out is None else out
        self._chk(self.lib.hp_dev_bfv_decrypt_round(self.h, n, L, _u64arr(moduli), t, B, self._ptr(x), self._ptr(out)))
        return out

    def poly_from_signed(self, moduli, coeffs):
        """small signed polynomials, coeffs [B][n] (any int64 values, device tensor) -> NTT form [B][L][n]: the words hp_dev_ntt produces
        from the strict residues.  How a ternary secret or an error polynomial gets to the device."""
        B, n = coeffs.shape
        L = len(moduli)
        out = self.empty((B, L, n))
        self._chk(self.lib.hp_dev_poly_from_signed(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(coeffs), self._ptr(out)))
        return out

    def hks_keygen(self, moduli_ext, k: int, alpha: int, s_to, s_from, a, e, out=None):
        """hybrid keys on the device: s_to [E][n], s_from [R][E][n], the uniform rows a [R][dnum][E][n] (NTT form, words < 2q) and the error
        polynomials e [R][dnum][n] (int64 coefficients) -> [R][dnum][2][E][n], canonical words.  a = None: the rows already lie in
        out[r][d][1] and are converted in place."""
        R, nd, n = e.shape
        E = len(moduli_ext)
        if out is None:
            if a is None:
                raise InvalidArgument(capi.HP_EINVAL, "hks_keygen: a = None needs the rows in out[..][1]")
            out = self.empty((R, nd, 2, E, n))
        self._chk(self.lib.hp_dev_hks_keygen(self.h, n.bit_length() - 1, E - k, k, alpha, _u64arr(moduli_ext), R, self._ptr(s_to),
                                             self._ptr(s_from), None if a is None else self._ptr(a), self._ptr(e), self._ptr(out)))
        return out

    def hks_keygen_rot(self, moduli_ext, k: int, alpha: int, s, steps, a, e, conj=None, out=None):
        """rotation / conjugation keys for the secret s [E][n]: key r switches move_r(s) back to s, move_r the cycle by steps[r] or (where
        conj[r]) the involution -- the key the rotate calls take for that entry.  a, e, out as for hks_keygen."""
        R, nd, n = e.shape
        E = len(moduli_ext)
        assert len(steps) == R and (conj is None or len(conj) == R)
        if out is None:
            if a is None:
                raise InvalidArgument(capi.HP_EINVAL, "hks_keygen_rot: a = None needs the rows in out[..][1]")
            out = self.empty((R, nd, 2, E, n))
        st = (C.c_size_t * R)(*[int(x) for x in steps])
        cj = (C.c_ubyte * R)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._chk(self.lib.hp_dev_hks_keygen_rot(self.h, n.bit_length() - 1, E - k, k, alpha, _u64arr(moduli_ext), R, st, cj, self._ptr(s),
                                                 None if a is None else self._ptr(a), self._ptr(e), self._ptr(out)))
        return out

    # -- device sampling: everything a function of (seed: 32 bytes, stream: 64-bit polynomial id) ----
    @staticmethod
    def _seed(seed: bytes):
        if len(seed) != 32:
            raise InvalidArgument(capi.HP_EINVAL, "a sampling seed is 32 bytes")
        return (C.c_ubyte * 32).from_buffer_copy(bytes(seed))

    def sample_uniform(self, logn: int, moduli, seed: bytes, stream: int, batch: int = 1, limb_ids=None, out=None, stride_words: int = 0):
        """uniform residues -> [batch][L][n], canonical words, directly as NTT-form rows; polynomial b has the id stream + b, row m the
        label limb_ids[m] (default m).  out with stride_words: polynomial b goes to out + b * stride_words words, the gaps untouched."""
        L, n = len(moduli), 1 << logn
        assert (out is None) == (stride_words == 0)
        out = self.empty((batch, L, n)) if out is None else out
        ids = None if limb_ids is None else (C.c_uint32 * L)(*[int(i) for i in limb_ids])
        self._chk(self.lib.hp_dev_sample_uniform(self.h, logn, L, _u64arr(moduli), ids, batch, self._seed(seed), stream, stride_words,
                                                 self._ptr(out)))
        return out

    def sample_ternary(self, logn: int, seed: bytes, stream: int, batch: int = 1):
        """ternary coefficients in {-1, 0, 1} -> int64 [batch][n] (poly_from_signed turns them into a secret's rows)"""
        out = self.empty((batch, 1 << logn))
        self._chk(self.lib.hp_dev_sample_ternary(self.h, logn, batch, self._seed(seed), stream, self._ptr(out)))
        return out

    def sample_cbd(self, logn: int, seed: bytes, stream: int, batch: int = 1):
        """centred binomial coefficients, eta = 21 (range +-21, variance 10.5) -> int64 [batch][n]"""
        out = self.empty((batch, 1 << logn))
        self._chk(self.lib.hp_dev_sample_cbd(self.h, logn, batch, self._seed(seed), stream, self._ptr(out)))
        return out

    def sample_gauss(self, logn: int, seed: bytes, stream: int, batch: int = 1):
        """discrete Gaussian coefficients, sigma = 3.2 (a 30-entry cumulative table: range +-30, variance 10.24) -> int64 [batch][n]"""
        out = self.empty((batch, 1 << logn))
        self._chk(self.lib.hp_dev_sample_gauss(self.h, logn, batch, self._seed(seed), stream, self._ptr(out)))
        return out

    def hks_keygen_seeded(self, moduli_ext, k: int, alpha: int, s_to, s_from, seed: bytes, stream: int, error_scale: int = 1, out=None):
        """hks_keygen on rows drawn on the device: for key r, digit d, a = the uniform sample and e = error_scale * the sample of the
        context's error sampler (set_error_sampler: centred binomial by default) of the polynomial id stream + r * dnum + d.  s_to [E][n], s_from [R][E][n] -> [R][dnum][2][E][n]."""
        R, E, n = s_from.shape
        nd = (E - k + alpha - 1) // alpha
        out = self.empty((R, nd, 2, E, n)) if out is None else out
        self._chk(self.lib.hp_dev_hks_keygen_seeded(self.h, n.bit_length() - 1, E - k, k, alpha, _u64arr(moduli_ext), R, self._ptr(s_to),
                                                    self._ptr(s_from), self._seed(seed), stream, error_scale, self._ptr(out)))
        return out

    def hks_keygen_rot_seeded(self, moduli_ext, k: int, alpha: int, s, steps, seed: bytes, stream: int, error_scale: int = 1, conj=None,
                              out=None):
        """hks_keygen_rot on rows drawn on the device (ids as for hks_keygen_seeded): s [E][n] -> [len(steps)][dnum][2][E][n]"""
        E, n = s.shape
        R = len(steps)
        assert conj is None or len(conj) == R
        nd = (E - k + alpha - 1) // alpha
        out = self.empty((R, nd, 2, E, n)) if out is None else out
        st = (C.c_size_t * R)(*[int(x) for x in steps])
        cj = (C.c_ubyte * R)(*[1 if c else 0 for c in conj]) if conj is not None else None
        self._chk(self.lib.hp_dev_hks_keygen_rot_seeded(self.h, n.bit_length() - 1, E - k, k, alpha, _u64arr(moduli_ext), R, st, cj,
                                                        self._ptr(s), self._seed(seed), stream, error_scale, self._ptr(out)))
        return out

    def hks_key_expand(self, moduli_ext, k: int, alpha: int, keys, seed: bytes, stream: int):
        """keys [R][dnum][2][E][n] whose [0] halves are loaded: the [1] halves are rewritten from (seed, stream), in place"""
        R, nd, _, E, n = keys.shape
        self._chk(self.lib.hp_dev_hks_key_expand(self.h, n.bit_length() - 1, E - k, k, alpha, _u64arr(moduli_ext), R, self._seed(seed),
                                                 stream, self._ptr(keys)))
        return keys

    def sample_small_ntt(self, logn: int, moduli, kind: int, seed: bytes, stream: int, batch: int = 1, scale: int = 1, out=None):
        """kind 2 (ternary) or 3 (centred binomial): scale * the sample of the polynomial id stream + b, in NTT form -> [batch][L][n],
        canonical words (poly_from_signed of the sampled rows, reduced), without the int64 rows.  A secret from 40 bytes."""
        L = len(moduli)
        out = self.empty((batch, L, 1 << logn)) if out is None else out
        self._chk(self.lib.hp_dev_sample_small_ntt(self.h, logn, L, _u64arr(moduli), batch, kind, self._seed(seed), stream, scale,
                                                   self._ptr(out)))
        return out

    def rlwe_encrypt_seeded(self, moduli, sk, pt, seed: bytes, stream: int, error_scale: int = 1, with_c1: bool = True, batch=None,
                            out=None):
        """secret-key encryption on rows drawn on the device: sk [L][n] (NTT form), pt [B][L][n] (coefficient form) or None (zero; then
        `batch` ciphertexts).  Ciphertext b: a = the uniform, e = error_scale * the error sampler's sample of the id stream + b;
        -> [B][2][L][n] = (e + pt - a s, a), or with_c1 = False [B][L][n]: c0 alone, the ciphertext being c0 + (seed, stream).
        pt = None with c1 is a public key (e - a s, a).  Canonical words."""
        L, n = sk.shape
        B = pt.shape[0] if pt is not None else (1 if batch is None else batch)
        assert pt is None or batch is None or batch == B
        out = self.empty((B, 2, L, n) if with_c1 else (B, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_rlwe_encrypt_seeded(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(sk),
                                                      None if pt is None else self._ptr(pt), self._seed(seed), stream, error_scale,
                                                      1 if with_c1 else 0, self._ptr(out)))
        return out

    def rlwe_encrypt_pk_seeded(self, moduli, pk, pt, seed: bytes, stream: int, error_scale: int = 1, batch=None, out=None):
        """public-key encryption: pk [2][L][n] (rlwe_encrypt_seeded with pt = None), pt [B][L][n] (coefficient form) or None.
        Ciphertext b: u = the ternary sample of the id stream + 2b, e0, e1 = error_scale * the error sampler's samples of stream + 2b,
        stream + 2b + 1 -> [B][2][L][n] = (pk0 u + e0 + pt, pk1 u + e1), canonical words.  Ids stream .. stream + 2B - 1."""
        _, L, n = pk.shape
        B = pt.shape[0] if pt is not None else (1 if batch is None else batch)
        assert pt is None or batch is None or batch == B
        out = self.empty((B, 2, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_rlwe_encrypt_pk_seeded(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(pk),
                                                         None if pt is None else self._ptr(pt), self._seed(seed), stream, error_scale,
                                                         self._ptr(out)))
        return out

    def ckks_rescale_n(self, moduli, ct, drops: int):
        B, _, L, n = ct.shape
        out = self.empty((B, 2, L - drops, n))
        tmp = self.empty((2, B, 2, L - 1, n)) if drops > 1 else None
        self._chk(self.lib.hp_dev_ckks_rescale_n(self.h, n.bit_length() - 1, L, _u64arr(moduli), drops, B, self._ptr(ct),
                                                 self._ptr(tmp) if tmp is not None else None, self._ptr(out)))
        return out

    # -- limb-range stages of the drop (the calls hehub_amd/sharded.py makes) ----
    def drop_coeffs(self, moduli, t: int, x):
        """x [..][L][n] -> the strict coefficients [P2][n] of every polynomial's last limb (t != 0: BGV, times t^-1)"""
        L, n = x.shape[-2:]
        P2 = x.numel() // (L * n)
        clast = self.empty((P2, n))
        self._chk(self.lib.hp_dev_drop_coeffs(self.h, n.bit_length() - 1, L, _u64arr(moduli), t, P2, self._ptr(x), self._ptr(clast)))
        return clast

    def drop_apply_range(self, moduli, t: int, x, clast, k0: int, k1: int, addend=None, add_mask: int = 0, strict: bool = False, out=None):
        """the drop of the last modulus on the limbs [k0, k1) of x [..][L][n] given the coefficient rows clast [P2][n] -> [P2][L-1][n]
        (only those limbs are written).  addend: [B][2][La][n], polynomial h of each ciphertext gets its rows where bit h of add_mask is
        set.  strict: the caller vouches that every word of clast is below the last modulus (hp_dev_drop_apply_range_strict)."""
        L, n = x.shape[-2:]
        P2 = x.numel() // (L * n)
        out = self.empty((P2, L - 1, n)) if out is None else out
        fn = self.lib.hp_dev_drop_apply_range_strict if strict else self.lib.hp_dev_drop_apply_range
        La = addend.shape[-2] if addend is not None else 0
        self._chk(fn(self.h, n.bit_length() - 1, L, _u64arr(moduli), t, P2, k0, k1, self._ptr(x), self._ptr(clast),
                     self._ptr(addend) if addend is not None else None, La, 2 * La, add_mask if addend is not None else 0, self._ptr(out)))
        return out

    # -- either side of the path -------------------------------------------
    def rlwe_encrypt_core(self, moduli, noise, c1, pt, sk):
        B, L, n = c1.shape
        ct = self.empty((B, 2, L, n))
        self._chk(self.lib.hp_dev_rlwe_encrypt_core(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(noise),
                                                    self._ptr(c1), self._ptr(pt), self._ptr(sk), self._ptr(ct)))
        return ct

    def rlwe_decrypt_core(self, moduli, ct, sk):
        B, _, L, n = ct.shape
        pt = self.empty((B, L, n))
        self._chk(self.lib.hp_dev_rlwe_decrypt_core(self.h, n.bit_length() - 1, L, _u64arr(moduli), B, self._ptr(ct),
                                                    self._ptr(sk), self._ptr(pt)))
        return pt

    def rns_base_from_single(self, old_modulus, new_moduli, x):
        B, n = x.shape
        L = len(new_moduli)
        out = self.empty((B, L, n))
        self._chk(self.lib.hp_dev_rns_base_from_single(self.h, n, old_modulus, L, _u64arr(new_moduli), B, self._ptr(x),
                                                       self._ptr(out)))
        return out

    def ckks_mod_raise(self, moduli, ct, out=None):
        """ModRaise (include/hehub_amd.h: hp_dev_ckks_mod_raise): ct [B][2][L_in][n] in NTT form, read at its limb row 0 (words
        below 2 q_0) -> [B][2][L][n] over moduli = q_0 .. q_{L-1}: row m >= 1 the transform modulo q_m of the centred coefficients
        of row 0, row 0 its canonical copy; residues, every word below 2 q_m."""
        B, two, Lin, n = ct.shape
        assert two == 2
        L = len(moduli)
        out = self.empty((B, 2, L, n)) if out is None else out
        self._chk(self.lib.hp_dev_ckks_mod_raise(self.h, n.bit_length() - 1, L, _u64arr(moduli), Lin, B, self._ptr(ct), self._ptr(out)))
        return out

    def rns_base_to_single_small(self, old_moduli, new_modulus, x):
        """returns (out[B][n], not_small[B]); not_small != 0 marks polynomials that need the host CRT branch."""
        B, L, n = x.shape
        out = self.empty((B, n))
        flags = self.torch.empty((B,), dtype=self.torch.int32, device=x.device)
        self._chk(self.lib.hp_dev_rns_base_to_single_small(self.h, n, L, _u64arr(old_moduli), new_modulus, B, self._ptr(x),
                                                           self._ptr(out), C.c_void_p(flags.data_ptr())))
        return out, flags

    def rns_base_to_single(self, old_moduli, new_modulus, x):
        """rns_base_transform(poly, {new_modulus}) complete: small-coefficient or CRT branch per polynomial."""
        B, L, n = x.shape
        out = self.empty((B, n))
        self._chk(self.lib.hp_dev_rns_base_to_single(self.h, n, L, _u64arr(old_moduli), new_modulus, B, self._ptr(x),
                                                     self._ptr(out)))
        return out

    def ckks_mult(self, moduli_ext, ct1, ct2, key, out=None):
        B, two, L, n = ct1.shape
        out = self.empty((B, 2, L - 1, n)) if out is None else out
        self._chk(self.lib.hp_dev_ckks_mult_relin_rescale(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), B,
                                                          self._ptr(ct1), self._ptr(ct2), self._ptr(key),
                                                          self._ptr(out)))
        return out

    def bgv_mult(self, moduli_ext, t, ct1, ct2, key, out=None, inner_t: bool = False):
        """inner_t: the extension that keeps the key-switched term (hp_dev_bgv_mult_relin_modswitch_t)"""
        B, two, L, n = ct1.shape
        out = self.empty((B, 2, L - 1, n)) if out is None else out
        fn = self.lib.hp_dev_bgv_mult_relin_modswitch_t if inner_t else self.lib.hp_dev_bgv_mult_relin_modswitch
        self._chk(fn(self.h, n.bit_length() - 1, L, _u64arr(moduli_ext), t, B,
                                                           self._ptr(ct1), self._ptr(ct2), self._ptr(key),
                                                           self._ptr(out)))
        return out
