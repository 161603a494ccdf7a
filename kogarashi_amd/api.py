"""Host-side mirror of the reference's call sites for the hot path (same names, argument meaning and error
behaviour), implemented on top of the C ABI.  Field elements are numpy uint64 arrays of 4 little-endian
Montgomery limbs (the reference's `Fr([u64; 4])` / `Fq`), points are (x | y) rows plus an infinity-flag array.

  msm_curve_addition(bases, coeffs)            groth16/src/msm.rs:6-48
  Fft(k).dft / idft / coset_dft / coset_idft / divide_by_z_on_coset      groth16/src/fft.rs:27-154
  PedersenCommitment(g).commit(m)              nova/src/pedersen.rs:10-20
  Prover(params).create_proof(...)             groth16/src/prover.rs:14-99
  NovaProver(shape, ck).compute_cross_term / commit_t      nova/src/prover.rs:24-90
"""
from __future__ import annotations

import numpy as np

from .lib import KG_CHECK_CURVE, KG_CHECK_SUBGROUP, KG_FQ, KG_FR, KG_G1, KG_G2, KG_GRUMPKIN, Context, Groth16Crs, KogarashiError

_default_ctx = None
CURVE_IDS = {"g1": KG_G1, "grumpkin": KG_GRUMPKIN, "gk": KG_GRUMPKIN, "g2": KG_G2}
_LIMBS = {KG_G1: 8, KG_GRUMPKIN: 8, KG_G2: 16}


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def msm_curve_addition(bases, coeffs, curve="g1", is_infinity=None, ctx: Context | None = None) -> np.ndarray:
    """Variable-base MSM over min(len(bases), len(coeffs)) pairs (the reference zips, msm.rs:25).
    Returns the projective sum as 3 base-field elements (x, y, z), normalised to z = 1 / (0, 1, 0)."""
    ctx = ctx or default_context()
    cid = CURVE_IDS[curve] if isinstance(curve, str) else int(curve)
    w = _LIMBS[cid]
    bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, w)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
    n = min(len(bases), len(coeffs))
    inf = None
    if is_infinity is not None:
        inf = np.ascontiguousarray(is_infinity, dtype=np.uint8)[:n]
    return ctx.msm_host(cid, bases[:n], inf, coeffs[:n], n)


def check_points(points, curve="g1", is_infinity=None, subgroup=True, ctx: Context | None = None) -> np.ndarray:
    """Status byte per point (kg_points_check): 0 = valid, KG_PT_NON_CANONICAL, KG_PT_OFF_CURVE, KG_PT_NOT_IN_SUBGROUP (G2 with
    subgroup=True: [r]P != O).  The reference's Group::is_on_curve / is_torsion_free (group.rs:59-65, bn254/src/g2.rs:26) over a whole
    array; what a host runs on a key or CRS of unknown origin before it hands it to PedersenCommitment / Prover."""
    ctx = ctx or default_context()
    cid = CURVE_IDS[curve] if isinstance(curve, str) else int(curve)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, _LIMBS[cid])
    n = len(pts)
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    d = ctx.upload(pts)
    di = ctx.upload(np.ascontiguousarray(is_infinity, dtype=np.uint8)[:n]) if is_infinity is not None else None
    st = ctx.empty((n,), dtype=np.uint8)
    ctx.points_check(cid, d.ptr, di.ptr if di else 0, n, KG_CHECK_CURVE | (KG_CHECK_SUBGROUP if subgroup else 0), st.ptr)
    return st.numpy()


class Fft:
    """groth16::fft::Fft<Fr>: size-2^k transforms, natural order in and out; inputs shorter than n are
    zero-padded like prepare_fft (fft.rs:157-162).  Unlike the reference, twiddles are cached on the device."""

    def __init__(self, k: int, ctx: Context | None = None):
        if k < 1:
            raise AssertionError("k >= 1")          # fft.rs:28 assert!(k >= 1)
        if k > 28:
            raise ValueError("k exceeds the two-adicity S = 28 of Fr")
        self.k, self.n = k, 1 << k
        self.ctx = ctx or default_context()

    def _run(self, v, inverse, coset):
        v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
        buf = np.zeros((self.n, 4), dtype=np.uint64)
        buf[: min(len(v), self.n)] = v[: self.n]
        d = self.ctx.upload(buf)
        self.ctx.ntt(d.ptr, self.k, inverse, coset)
        return d.numpy()

    def dft(self, coeffs):
        return self._run(coeffs, False, False)

    def idft(self, points):
        return self._run(points, True, False)

    def coset_dft(self, coeffs):
        return self._run(coeffs, False, True)

    def coset_idft(self, points):
        return self._run(points, True, True)

    def divide_by_z_on_coset(self, points):
        v = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        buf = np.zeros((self.n, 4), dtype=np.uint64)
        buf[: min(len(v), self.n)] = v[: self.n]
        d = self.ctx.upload(buf)
        self.ctx.divide_by_z_on_coset(d.ptr, self.k)
        return d.numpy()

    def _rows(self, vs):
        """B polynomials (a (B, <= n, 4) array or a list of (<= n, 4) arrays) -> a zero-padded (B, n, 4) array, each row like _run"""
        buf = np.zeros((len(vs), self.n, 4), dtype=np.uint64)
        for b, v in enumerate(vs):
            v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
            buf[b, : min(len(v), self.n)] = v[: self.n]
        return buf

    def batch(self, vs, inverse=False, coset=False):
        """every row of vs through one transform (dft / idft / coset_dft / coset_idft by the two flags) in a single call
        (kg_ntt_bn254_fr_batch): (B, <= n, 4) in, (B, n, 4) out"""
        buf = self._rows(vs)
        if len(buf) == 0:
            return buf
        d = self.ctx.upload(buf.reshape(-1, 4))
        self.ctx.ntt_batch(d.ptr, self.k, len(buf), self.n, inverse, coset)
        return d.numpy().reshape(len(buf), self.n, 4)

    def divide_by_z_on_coset_batch(self, vs):
        buf = self._rows(vs)
        if len(buf) == 0:
            return buf
        d = self.ctx.upload(buf.reshape(-1, 4))
        self.ctx.divide_by_z_on_coset_batch(d.ptr, self.k, len(buf), self.n)
        return d.numpy().reshape(len(buf), self.n, 4)


class PedersenCommitment:
    """nova::PedersenCommitment<C>: commit(m) = affine(sum_i g[i] * m[i]) over min(len) pairs.
    The generators are uploaded once and stay resident (the reference re-reads them on every call)."""

    def __init__(self, g, curve="g1", is_infinity=None, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.cid = CURVE_IDS[curve] if isinstance(curve, str) else int(curve)
        w = _LIMBS[self.cid]
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, w)
        self.len = len(g)
        self._g = self.ctx.upload(g)
        self._inf = None
        if is_infinity is not None:
            self._inf = self.ctx.upload(np.ascontiguousarray(is_infinity, dtype=np.uint8))
        self.ctx.bases_register(self.cid, self._g.ptr, self._inf.ptr if self._inf else 0, self.len)

    def __del__(self):
        try:
            self.ctx.bases_unregister(self._g.ptr)
        except Exception:
            pass

    def check(self, subgroup: bool = True) -> tuple[int, int]:
        """(bad, first_bad) of kg_points_check over the resident generators: (0, len) for a key every point of which is on the curve
        (and, for G2 with subgroup=True, in the order-r subgroup)"""
        return self.ctx.points_check(self.cid, self._g.ptr, self._inf.ptr if self._inf else 0, self.len,
                                     KG_CHECK_CURVE | (KG_CHECK_SUBGROUP if subgroup else 0))

    def commit(self, m):
        m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1, 4)
        n = min(len(m), self.len)
        # the key is resident, m is a host slice: uploaded in index slices under the accumulations (kg_commit_host_scalars)
        return self.ctx.commit_host_scalars(self.cid, self._g.ptr, self._inf.ptr if self._inf else 0, m[:n], n)

    def commit_batch(self, ms):
        """Commitments of several vectors of ONE length against this key in one call (kg_commit_batch): ms is a list of equal-length
        vectors or an array of shape (count, len, 4).  Returns (points, flags): arrays of shape (count, 8 | 16) and (count,); point b
        equals commit(ms[b]) bit for bit, the identity is (0, 1) with flag 1."""
        ms = np.ascontiguousarray(ms, dtype=np.uint64)
        if ms.ndim == 2 and ms.shape[1] == 4:
            raise ValueError("commit_batch takes a list of vectors or a (count, len, 4) array; use commit for one vector")
        count = ms.shape[0]
        ms = ms.reshape(count, -1, 4)
        length = ms.shape[1]
        n = min(length, self.len)
        w = _LIMBS[self.cid]
        if count == 0:
            return np.zeros((0, w), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
        d_m = self.ctx.upload(ms)
        d_xy, d_inf = self.ctx.empty((count, w)), self.ctx.empty((count,), dtype=np.uint8)
        self.ctx.commit_batch(self.cid, self._g.ptr, self._inf.ptr if self._inf else 0, d_m.ptr, n, count, length, d_xy.ptr, d_inf.ptr)
        return d_xy.numpy(), d_inf.numpy()      # (kg_memcpy_d2h follows the stream)


class Prover:
    """groth16::Prover { params }: the CRS (groth16/src/params.rs:6-28) is uploaded once and stays resident.

    params: dict with "h", "l", "a", "b_g1" (G1 rows x|y), "b_g2" (G2 rows), optional "<name>_inf" flag arrays,
    "vk_g1" = rows alpha_g1, beta_g1, delta_g1 and "vk_g2" = rows beta_g2, delta_g2 (affine), optional
    "delta_g1_inf"/"delta_g2_inf".

    window_tables=True additionally stores every vector's window multiples (kg_bases_precompute: ceil(255 / 17) = 15 x the
    CRS in device memory, built once): the five MSMs of a proof then use one bucket set each.  Offered for circuits whose
    witness and h vectors hold 2^16 .. 2^20 entries; other sizes keep the plain resident form."""

    def __init__(self, params: dict, m: int, l: int, m_l_1: int, ctx: Context | None = None, window_tables: bool = False):
        self.ctx = ctx or default_context()
        self.m, self.l, self.m_l_1 = m, l, m_l_1
        self._keep = []
        self._registered = []
        crs = Groth16Crs()
        crs.m, crs.l, crs.m_l_1 = m, l, m_l_1
        for name, w in (("h", 8), ("l", 8), ("a", 8), ("b_g1", 8), ("b_g2", 16)):
            arr = np.ascontiguousarray(params[name], dtype=np.uint64).reshape(-1, w)
            d = self.ctx.upload(arr)
            self._keep.append(d)
            setattr(crs, "d_" + name, d.ptr)
            inf = params.get(name + "_inf")
            di = None
            if inf is not None and np.any(inf):
                di = self.ctx.upload(np.ascontiguousarray(inf, dtype=np.uint8))
                self._keep.append(di)
                setattr(crs, "d_" + name + "_inf", di.ptr)
            # Parameters is immutable: convert each CRS vector to the device's internal form once
            self.ctx.bases_register(KG_G2 if w == 16 else KG_G1, d.ptr, di.ptr if di else 0, len(arr))
            self._registered.append(d.ptr)
        g1 = np.ascontiguousarray(params["vk_g1"], dtype=np.uint64).reshape(-1, 8)
        g2 = np.ascontiguousarray(params["vk_g2"], dtype=np.uint64).reshape(-1, 16)
        for i in range(8):
            crs.alpha_g1[i], crs.beta_g1[i], crs.delta_g1[i] = int(g1[0, i]), int(g1[1, i]), int(g1[2, i])
        for i in range(16):
            crs.beta_g2[i], crs.delta_g2[i] = int(g2[0, i]), int(g2[1, i])
        crs.delta_g1_inf = int(bool(params.get("delta_g1_inf", 0)))
        crs.delta_g2_inf = int(bool(params.get("delta_g2_inf", 0)))
        self.crs = crs
        self.window_tables = False
        nz, hn = l + m_l_1, m - 1
        if window_tables and all((1 << 16) <= v <= (1 << 20) for v in (nz, hn)) and len(params["h"]) == hn:
            for name in ("a", "b_g1", "b_g2", "l"):
                self.ctx.bases_precompute(getattr(crs, "d_" + name), nz)      # l meets the whole witness vector z = x || w
            self.ctx.bases_precompute(crs.d_h, hn)
            self.window_tables = True

    def __del__(self):
        for p_ in getattr(self, "_registered", []):
            try:
                self.ctx.bases_unregister(p_)
            except Exception:
                pass

    def check_crs(self, subgroup: bool = True) -> dict:
        """kg_groth16_crs_check over the resident CRS: {member: number of invalid points}, all zero for a CRS to trust"""
        return self.ctx.groth16_crs_check(self.crs, KG_CHECK_CURVE | (KG_CHECK_SUBGROUP if subgroup else 0))

    def create_proof(self, a_eval, b_eval, c_eval, x, w, r, s):
        """Proof {a, b, c} for the synthesised constraint system: (A, B, C) = cs.evaluate(), x = cs.x(), w = cs.w();
        (r, s) are the blinding scalars the reference draws from its rng (prover.rs:71-72).
        Raises ProverSubVersionCrsAttack like prover.rs:67-69."""
        up = lambda v: self.ctx.upload(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4))
        da, db, dc, dx, dw = up(a_eval), up(b_eval), up(c_eval), up(x), up(w)
        return self.ctx.groth16_prove(self.crs, da.ptr, db.ptr, dc.ptr, dx.ptr, dw.ptr, r, s)

    def attach_constraint_system(self, a, b, c):
        """The circuit's constraint matrices (CSR triples (row_ptr, col, val) over z = x || w, cs.matrices()): uploaded once;
        create_proof_from_witness then runs cs.evaluate() (zkstd/src/r1cs.rs:137-142) on the device as well."""
        self._cs = []
        for rp, col, val in (a, b, c):
            val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
            col = np.ascontiguousarray(col, dtype=np.uint64)
            self._cs.append((self.ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)),
                             self.ctx.upload(col if len(col) else np.zeros(1, dtype=np.uint64)),
                             self.ctx.upload(val if len(val) else np.zeros((1, 4), dtype=np.uint64))))

    def check_witness(self, x, w) -> tuple[int, int]:
        """R1cs::is_sat (zkstd/src/r1cs.rs:62-77) for z = x || w against the attached constraint system: (number of violated constraints,
        index of the first or m).  create_proof_from_witness does not run it: for a witness that violates a constraint it returns a
        well-formed proof that no verifier accepts."""
        up = lambda v: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
        dz = self.ctx.upload(np.concatenate([up(x), up(w)]))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._cs]
        return self.ctx.r1cs_check(KG_FR, ptrs[0], ptrs[1], ptrs[2], self.m, dz.ptr)

    def create_proof_from_witness(self, x, w, r, s):
        """create_proof from (x, w) alone: the evaluation vectors are made on the device (kg_groth16_prove_r1cs_bn254)"""
        up = lambda v: self.ctx.upload(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4))
        dx, dw = up(x), up(w)
        ptrs = [tuple(d.ptr for d in trip) for trip in self._cs]
        return self.ctx.groth16_prove_r1cs(self.crs, ptrs[0], ptrs[1], ptrs[2], dx.ptr, dw.ptr, r, s)

    def create_proofs(self, jobs):
        """Proofs for an iterable of (a_eval, b_eval, c_eval, x, w, r, s), two in flight (kg_groth16_prove_begin / _end):
        proof i+1 is enqueued before proof i is collected, so its transforms and sorts overlap proof i's last reduction
        and host assembly.  Yields the proofs in order."""
        up = lambda v: self.ctx.upload(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4))
        held = [None, None]
        in_flight = []                                  # tickets begun and not yet ended, oldest first
        try:
            for i, (a_eval, b_eval, c_eval, x, w, r, s) in enumerate(jobs):
                t = i & 1
                held[t] = [up(a_eval), up(b_eval), up(c_eval), up(x), up(w)]       # alive until the matching end
                da, db, dc, dx, dw = held[t]
                self.ctx.groth16_prove_begin(self.crs, da.ptr, db.ptr, dc.ptr, dx.ptr, dw.ptr, r, s, t)
                in_flight.append(t)
                if len(in_flight) == 2:
                    yield self.ctx.groth16_prove_end(in_flight.pop(0))
            while in_flight:
                yield self.ctx.groth16_prove_end(in_flight.pop(0))
        finally:
            for t in in_flight:                         # an error or an abandoned generator: every begin gets its end
                try:
                    self.ctx.groth16_prove_end(t)
                except Exception:
                    pass


    def create_proofs_batch(self, jobs):
        """Proofs for a list of (a_eval, b_eval, c_eval, x, w, r, s) of this circuit in ONE call (kg_groth16_prove_batch): the inputs are
        uploaded as packed arrays, every launch is shared by a group of proofs and the assembly runs on the device.  Returns
        (proofs, flags): arrays of shape (count, 32) -- A (8) | B (16) | C (8) words -- and (count, 3); proof b equals
        create_proof(*jobs[b]) bit for bit.  Raises KogarashiError (unsupported) for circuits whose MSMs are longer than the batched
        short MSM takes (lib.groth16_prove_batch_plan == (0, 0)): create_proofs is the loop for those."""
        jobs = list(jobs)
        count = len(jobs)
        if count == 0:
            return np.zeros((0, 32), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint8)
        pack = lambda k, n: np.ascontiguousarray(np.stack([np.asarray(j[k], dtype=np.uint64).reshape(-1, 4)[:n].reshape(n, 4) for j in jobs]))
        up = lambda a: self.ctx.upload(a if a.size else np.zeros((1, 4), dtype=np.uint64))
        da, db, dc = up(pack(0, self.m)), up(pack(1, self.m)), up(pack(2, self.m))
        dx, dw = up(pack(3, self.l)), up(pack(4, self.m_l_1))
        dr, ds = up(pack(5, 1)), up(pack(6, 1))
        d_out, d_inf = self.ctx.empty((count, 32)), self.ctx.empty((count, 3), dtype=np.uint8)
        self.ctx.groth16_prove_batch(self.crs, da.ptr, db.ptr, dc.ptr, self.m, dx.ptr, self.l, dw.ptr if self.m_l_1 else 0, self.m_l_1,
                                     dr.ptr, ds.ptr, count, d_out.ptr, d_inf.ptr)
        return d_out.numpy(), d_inf.numpy()      # (kg_memcpy_d2h follows the stream)

    def _upload_witnesses(self, jobs):
        """the first two members of every job, (x, w), as the packed device arrays the batch entries read (strides l and m_l_1)"""
        pack = lambda k, n: np.ascontiguousarray(np.stack([np.asarray(j[k], dtype=np.uint64).reshape(-1, 4)[:n].reshape(n, 4) for j in jobs]))
        up = lambda a: self.ctx.upload(a if a.size else np.zeros((1, 4), dtype=np.uint64))
        return up(pack(0, self.l)), up(pack(1, self.m_l_1))

    def _check_uploaded(self, dx, dw, count):
        ptrs = [tuple(d.ptr for d in trip) for trip in self._cs]
        return self.ctx.groth16_witness_check_batch(ptrs[0], ptrs[1], ptrs[2], self.m, self.l, self.m_l_1, dx.ptr, self.l,
                                                    dw.ptr if self.m_l_1 else 0, self.m_l_1, count)

    def check_witnesses(self, jobs) -> np.ndarray:
        """check_witness for a list of jobs whose first two members are (x, w), in ONE call (kg_groth16_witness_check_batch): x and w are
        uploaded as the batch prover takes them and read in place.  Returns an array (count, 2) of (number of violated constraints, index of
        the first or m) per witness."""
        if not hasattr(self, "_cs"):
            raise KogarashiError("check_witnesses needs attach_constraint_system first")
        jobs = list(jobs)
        if not jobs:
            return np.zeros((0, 2), dtype=np.uint32)
        dx, dw = self._upload_witnesses(jobs)
        return self._check_uploaded(dx, dw, len(jobs)).numpy()

    def create_proofs_batch_from_witness(self, jobs, check=False):
        """create_proofs_batch from witnesses alone: jobs are (x, w, r, s), the evaluation vectors of every proof are made on the device
        from the attached constraint system (attach_constraint_system; kg_groth16_prove_r1cs_batch).  Returns the same (proofs, flags) of
        shape (count, 32) and (count, 3); proof b equals create_proof_from_witness(*jobs[b]) bit for bit.
        check=True enqueues kg_groth16_witness_check_batch on the uploaded x and w in front of the proving call and returns
        (proofs, flags, summary), summary as check_witnesses returns it: proofs and flags are the same bits, a witness with summary[b, 0] != 0
        has a proof no verifier accepts."""
        if not hasattr(self, "_cs"):
            raise KogarashiError("create_proofs_batch_from_witness needs attach_constraint_system first")
        jobs = list(jobs)
        count = len(jobs)
        if count == 0:
            empty = (np.zeros((0, 32), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint8))
            return empty + (np.zeros((0, 2), dtype=np.uint32),) if check else empty
        pack = lambda k, n: np.ascontiguousarray(np.stack([np.asarray(j[k], dtype=np.uint64).reshape(-1, 4)[:n].reshape(n, 4) for j in jobs]))
        up = lambda a: self.ctx.upload(a if a.size else np.zeros((1, 4), dtype=np.uint64))
        dx, dw = self._upload_witnesses(jobs)
        dr, ds = up(pack(2, 1)), up(pack(3, 1))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._cs]
        d_out, d_inf = self.ctx.empty((count, 32)), self.ctx.empty((count, 3), dtype=np.uint8)
        d_sum = self._check_uploaded(dx, dw, count) if check else None
        self.ctx.groth16_prove_r1cs_batch(self.crs, ptrs[0], ptrs[1], ptrs[2], dx.ptr, self.l, dw.ptr if self.m_l_1 else 0, self.m_l_1,
                                          dr.ptr, ds.ptr, count, d_out.ptr, d_inf.ptr)
        out = (d_out.numpy(), d_inf.numpy())
        return out + (d_sum.numpy(),) if check else out


class ShardedProver:
    """groth16::Prover over several contexts (normally one per GPU), task-parallel: SURVEY.md 8e -- the MSMs of
    prover.rs:51-65 are independent until the assembly and the G2 query is the long pole.  Context 0 holds b_g2 and runs
    that query, context 1 % n holds a, b_g1, l (the three G1 queries against z = x || w), context 2 % n holds h and runs the
    transforms and h's MSM (kg_groth16_prove_sharded); each vector is uploaded and registered only where it is used."""

    ROLE_VECTORS = (("b_g2",), ("a", "b_g1", "l"), ("h",))

    def __init__(self, params: dict, m: int, l: int, m_l_1: int, ctxs):
        from .lib import groth16_prove_sharded
        self._prove = groth16_prove_sharded
        self.ctxs = list(ctxs)
        n = len(self.ctxs)
        self.owner = [0, 1 % n, 2 % n]
        self.m, self.l, self.m_l_1 = m, l, m_l_1
        self._keep, self._registered = [], []
        g1 = np.ascontiguousarray(params["vk_g1"], dtype=np.uint64).reshape(-1, 8)
        g2 = np.ascontiguousarray(params["vk_g2"], dtype=np.uint64).reshape(-1, 16)
        self.crs = []
        for ci, ctx in enumerate(self.ctxs):
            crs = Groth16Crs()
            crs.m, crs.l, crs.m_l_1 = m, l, m_l_1
            for role, names in enumerate(self.ROLE_VECTORS):
                if self.owner[role] != ci:
                    continue
                for name in names:
                    w = 16 if name == "b_g2" else 8
                    arr = np.ascontiguousarray(params[name], dtype=np.uint64).reshape(-1, w)
                    d = ctx.upload(arr)
                    self._keep.append(d)
                    setattr(crs, "d_" + name, d.ptr)
                    inf = params.get(name + "_inf")
                    di = None
                    if inf is not None and np.any(inf):
                        di = ctx.upload(np.ascontiguousarray(inf, dtype=np.uint8))
                        self._keep.append(di)
                        setattr(crs, "d_" + name + "_inf", di.ptr)
                    ctx.bases_register(KG_G2 if w == 16 else KG_G1, d.ptr, di.ptr if di else 0, len(arr))
                    self._registered.append((ctx, d.ptr))
            for i in range(8):
                crs.alpha_g1[i], crs.beta_g1[i], crs.delta_g1[i] = int(g1[0, i]), int(g1[1, i]), int(g1[2, i])
            for i in range(16):
                crs.beta_g2[i], crs.delta_g2[i] = int(g2[0, i]), int(g2[1, i])
            crs.delta_g1_inf = int(bool(params.get("delta_g1_inf", 0)))
            crs.delta_g2_inf = int(bool(params.get("delta_g2_inf", 0)))
            self.crs.append(crs)

    def __del__(self):
        for ctx, p_ in getattr(self, "_registered", []):
            try:
                ctx.bases_unregister(p_)
            except Exception:
                pass

    def create_proof(self, a_eval, b_eval, c_eval, x, w, r, s):
        """as Prover.create_proof; the witness goes to the contexts that run the queries against z, the evaluation vectors to
        the one that runs the transforms"""
        n = len(self.ctxs)
        up = lambda ctx, v: ctx.upload(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4))
        keep, ptr = [], {k: [0] * n for k in "abcxw"}
        for ci, ctx in enumerate(self.ctxs):
            if ci in self.owner[:2]:
                for k, v in (("x", x), ("w", w)):
                    d = up(ctx, v)
                    keep.append(d)
                    ptr[k][ci] = d.ptr
            if ci == self.owner[2]:
                for k, v in (("a", a_eval), ("b", b_eval), ("c", c_eval)):
                    d = up(ctx, v)
                    keep.append(d)
                    ptr[k][ci] = d.ptr
        return self._prove(self.ctxs, self.crs, ptr["a"], ptr["b"], ptr["c"], ptr["x"], ptr["w"], r, s)

    def upload_inputs(self, a_eval, b_eval, c_eval, x, w):
        """the inputs of create_proof made resident where they are read (returns the per-context pointer lists and the arrays
        that keep them alive): repeated proofs over the same inputs then move nothing over PCIe (bench.py groth16.sharded)"""
        n = len(self.ctxs)
        up = lambda ctx, v: ctx.upload(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4))
        keep, ptr = [], {k: [0] * n for k in "abcxw"}
        for ci, ctx in enumerate(self.ctxs):
            if ci in self.owner[:2]:
                for k, v in (("x", x), ("w", w)):
                    d = up(ctx, v)
                    keep.append(d)
                    ptr[k][ci] = d.ptr
            if ci == self.owner[2]:
                for k, v in (("a", a_eval), ("b", b_eval), ("c", c_eval)):
                    d = up(ctx, v)
                    keep.append(d)
                    ptr[k][ci] = d.ptr
        return ptr, keep

    def prove_resident(self, ptr, r, s):
        return self._prove(self.ctxs, self.crs, ptr["a"], ptr["b"], ptr["c"], ptr["x"], ptr["w"], r, s)



class NovaProver:
    """nova::Prover { ck, shape } as far as the hot path goes: the cross term T of a folding step and its commitment
    (nova/src/prover.rs:31-35, 53-90).  shape: the R1CS matrices (a, b, c) as CSR triples (row_ptr, col, val) over
    z = (u | x | w) -- column 0 is the relaxed one-wire, instance wire i is column i, witness wire k is column l + k with
    l = len(x) + 1 (SparseMatrix::prod's index rule, zkstd/src/matrix.rs:36-48).  Scalars are Fr for the bn254 driver and
    Fq for the Grumpkin driver (nova/src/driver.rs:9-42).  The matrices are uploaded once and stay resident."""

    def __init__(self, shape, ck: "PedersenCommitment", ctx: Context | None = None):
        self.ctx = ctx or ck.ctx
        self.ck = ck
        self.field = KG_FQ if ck.cid == KG_GRUMPKIN else KG_FR
        self.m = len(shape[0][0]) - 1
        self._dev = []
        for rp, col, val in shape:
            val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
            col = np.ascontiguousarray(col, dtype=np.uint64)
            self._dev.append((self.ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)),
                              self.ctx.upload(col if len(col) else np.zeros(1, dtype=np.uint64)),
                              self.ctx.upload(val if len(val) else np.zeros((1, 4), dtype=np.uint64))))

    def _z(self, u, x, w):
        parts = [np.ascontiguousarray(u, dtype=np.uint64).reshape(1, 4), np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4),
                 np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)]
        return self.ctx.upload(np.concatenate(parts))

    def compute_cross_term_device(self, u1, x1, w1, u2, x2, w2):
        """T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - u2 CZ1 as a device array of m elements (prover.rs:53-90)"""
        z1, z2 = self._z(u1, x1, w1), self._z(u2, x2, w2)
        t = self.ctx.empty((self.m, 4))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._dev]
        self.ctx.nova_cross_term(self.field, ptrs[0], ptrs[1], ptrs[2], self.m, z1.ptr, z2.ptr, u1, u2, t.ptr)
        return t

    def compute_cross_term(self, u1, x1, w1, u2, x2, w2) -> np.ndarray:
        return self.compute_cross_term_device(u1, x1, w1, u2, x2, w2).numpy()

    def _one(self):
        """the scalar field's one in Montgomery form, made by the device (to_mont of the integer 1)"""
        if getattr(self, "_one_cache", None) is None:
            d = self.ctx.upload(np.array([[1, 0, 0, 0]], dtype=np.uint64))
            self.ctx.field_vec_op(self.field, "to_mont", d.ptr, 0, d.ptr, 1)
            self._one_cache = d.numpy()[0].copy()
        return self._one_cache

    def prove(self, instance1: dict, witness1: dict, instance2: dict, witness2: dict, r):
        """nova::Prover::prove (nova/src/prover.rs:24-50) with the challenge r supplied by the caller -- the transcript hash
        that produces it is sequential host work outside the hot path.

        instance1: relaxed instance {"commit_w": (xy, inf), "commit_e": (xy, inf), "u": limbs, "x": (k, 4)};
        witness1: {"w": (n, 4), "e": (m, 4)}; instance2: {"commit_w": (xy, inf), "x": (k, 4)}; witness2: {"w": (n, 4)}.
        Returns (instance, witness, commit_t) in the same shapes.  On the device: the cross term, its commitment and both
        witness folds (W1 + r W2, E1 + r T: relaxed_r1cs/witness.rs:56-70); the instance fold (instance.rs:81-101) is two
        two-point MSMs and a handful of scalars."""
        c, fd, cid = self.ctx, self.field, self.ck.cid
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(4)
        one = self._one()
        u1 = np.ascontiguousarray(instance1["u"], dtype=np.uint64).reshape(4)
        x1 = np.ascontiguousarray(instance1["x"], dtype=np.uint64).reshape(-1, 4)
        x2 = np.ascontiguousarray(instance2["x"], dtype=np.uint64).reshape(-1, 4)
        w1 = np.ascontiguousarray(witness1["w"], dtype=np.uint64).reshape(-1, 4)
        w2 = np.ascontiguousarray(witness2["w"], dtype=np.uint64).reshape(-1, 4)
        t = self.compute_cross_term_device(u1, x1, w1, one, x2, w2)
        n = min(self.m, self.ck.len)
        commit_t = c.commit(cid, self.ck._g.ptr, self.ck._inf.ptr if self.ck._inf else 0, t.ptr, n)
        # witness fold
        dw1, dw2, de1 = c.upload(w1), c.upload(w2), c.upload(np.ascontiguousarray(witness1["e"], dtype=np.uint64).reshape(-1, 4))
        c.field_vec_axpy(fd, dw1.ptr, r, dw2.ptr, dw1.ptr, len(w1))
        c.field_vec_axpy(fd, de1.ptr, r, t.ptr, de1.ptr, self.m)
        # instance fold: u = u1 + r, x = x1 + r x2 (one small axpy over u | x against 1 | x2)
        ux1, ux2 = c.upload(np.concatenate([u1.reshape(1, 4), x1])), c.upload(np.concatenate([one.reshape(1, 4), x2]))
        c.field_vec_axpy(fd, ux1.ptr, r, ux2.ptr, ux1.ptr, 1 + len(x1))
        ux = ux1.numpy()

        def fold_point(p1, p2):                     # p1 + r * p2 as an affine point: msm([p1, p2], [1, r])
            w = 16 if cid == KG_G2 else 8
            pts = np.stack([np.ascontiguousarray(p1[0], dtype=np.uint64).reshape(w), np.ascontiguousarray(p2[0], dtype=np.uint64).reshape(w)])
            flags = np.array([int(bool(p1[1])), int(bool(p2[1]))], dtype=np.uint8)
            out = c.msm_host(cid, pts, flags, np.stack([one, r]), 2)
            return out[:w].copy(), int(not out[w:].any())

        instance = {"commit_w": fold_point(instance1["commit_w"], instance2["commit_w"]),
                    "commit_e": fold_point(instance1["commit_e"], commit_t), "u": ux[0].copy(), "x": ux[1:].copy()}
        return instance, {"w": dw1.numpy(), "e": de1.numpy()}, commit_t

    # ---- a batch of folds: two enqueued phases with the transcript's challenges in between --------------------------------------------
    def fold_begin(self, pairs):
        """The first phase of prove() for a list of (instance1, witness1, instance2, witness2) in the dict shapes prove() takes, all of
        this shape: the z1 = (u | x1 | w1), z2 = (1 | x2 | w2) and E1 arrays are packed and uploaded once, the cross terms
        (kg_nova_cross_term_batch) and their commitments (kg_commit_batch over the T rows, n = min(m, len(ck))) are enqueued, and only
        the count commitments are read back.  Returns (state, commit_ts): commit_ts is the list of (xy, inf) the caller's transcript
        hashes into the challenges fold_end takes; state is handed to fold_end unchanged.
        Beyond 2048 constraints kg_commit_batch runs its blocking loop of single commitments (kg_commit_batch_plan reports 0 groups):
        the result is the same, the commitments are then not one launch group."""
        c, fd, cid, m = self.ctx, self.field, self.ck.cid, self.m
        pairs = list(pairs)
        count = len(pairs)
        if count == 0:
            return {"count": 0}, []
        el = lambda v: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
        one = self._one()
        z1 = np.ascontiguousarray(np.stack([np.concatenate([el(i1["u"]), el(i1["x"]), el(w1["w"])]) for i1, w1, _, _ in pairs]))
        z2 = np.ascontiguousarray(np.stack([np.concatenate([one.reshape(1, 4), el(i2["x"]), el(w2["w"])]) for _, _, i2, w2 in pairs]))
        if z1.shape != z2.shape:
            raise ValueError("the two sides of a fold have different numbers of instance or witness values")
        e1 = np.ascontiguousarray(np.stack([el(w1["e"]) for _, w1, _, _ in pairs]))
        if e1.shape[1] != m:
            raise ValueError("an error vector whose length is not the shape's number of constraints")
        nz, lx = z1.shape[1], len(el(pairs[0][0]["x"]))
        dz1, dz2, de1, du1, dt = c.upload(z1), c.upload(z2), c.upload(e1), c.upload(np.ascontiguousarray(z1[:, 0])), c.empty((count, max(m, 1), 4))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._dev]
        c.nova_cross_term_batch(fd, ptrs[0], ptrs[1], ptrs[2], m, dz1.ptr, nz, dz2.ptr, nz, count, du1.ptr, 0, dt.ptr, m)
        n = min(m, self.ck.len)
        d_ct, d_ct_inf = c.empty((count, 8)), c.empty((count,), dtype=np.uint8)
        c.commit_batch(cid, self.ck._g.ptr, self.ck._inf.ptr if self.ck._inf else 0, dt.ptr, n, count, m, d_ct.ptr, d_ct_inf.ptr)
        ct, ct_inf = d_ct.numpy(), d_ct_inf.numpy()              # the one read-back of the phase: count points
        # the point fold's operands, interleaved per pair: P = (commit_w1, commit_e1), Q = (commit_w2, commit_T)
        pxy, qxy = np.zeros((2 * count, 8), dtype=np.uint64), np.zeros((2 * count, 8), dtype=np.uint64)
        pinf, qinf = np.zeros(2 * count, dtype=np.uint8), np.zeros(2 * count, dtype=np.uint8)
        for b, (i1, _, i2, _) in enumerate(pairs):
            for dst, dinf, j, pt in ((pxy, pinf, 2 * b, i1["commit_w"]), (pxy, pinf, 2 * b + 1, i1["commit_e"]), (qxy, qinf, 2 * b, i2["commit_w"])):
                dinf[j] = int(bool(pt[1]))
                if not dinf[j]:
                    dst[j] = np.ascontiguousarray(pt[0], dtype=np.uint64).reshape(8)
            qxy[2 * b + 1], qinf[2 * b + 1] = ct[b], ct_inf[b]
        state = {"count": count, "nz": nz, "lx": lx, "z1": dz1, "z2": dz2, "e1": de1, "t": dt, "pxy": c.upload(pxy), "pinf": c.upload(pinf),
                 "qxy": c.upload(qxy), "qinf": c.upload(qinf), "commit_t": [(ct[b].copy(), int(ct_inf[b])) for b in range(count)]}
        return state, state["commit_t"]

    def fold_end(self, state, rs):
        """The second phase: rs is a (count, 4) array of challenges, one per pair of fold_begin.  Uploads them and enqueues z1 += r z2
        (u, x and W in one pass: z = (u | x | w) and z2 begins with one), E1 += r T (kg_field_vec_axpy_batch) and the 2 count point folds
        (commit_w1 + r commit_w2, commit_e1 + r commit_T: kg_points_muladd_batch, per_scalar = 2); then reads the folded pairs back.
        Returns the list of (instance, witness, commit_t) in prove()'s shapes."""
        c, fd, cid, m = self.ctx, self.field, self.ck.cid, self.m
        count = state["count"]
        if count == 0:
            return []
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(count, 4)
        dr = c.upload(rs)
        nz, lx = state["nz"], state["lx"]
        c.field_vec_axpy_batch(fd, state["z1"].ptr, nz, dr.ptr, state["z2"].ptr, nz, state["z1"].ptr, nz, nz, count)
        c.field_vec_axpy_batch(fd, state["e1"].ptr, m, dr.ptr, state["t"].ptr, m, state["e1"].ptr, m, m, count)
        c.points_muladd_batch(cid, state["pxy"].ptr, state["pinf"].ptr, state["qxy"].ptr, state["qinf"].ptr, dr.ptr, 2, 2 * count, state["pxy"].ptr,
                              state["pinf"].ptr)
        z, e, xy, inf = state["z1"].numpy(), state["e1"].numpy(), state["pxy"].numpy(), state["pinf"].numpy()
        out = []
        for b in range(count):
            instance = {"commit_w": (xy[2 * b].copy(), int(inf[2 * b])), "commit_e": (xy[2 * b + 1].copy(), int(inf[2 * b + 1])),
                        "u": z[b, 0].copy(), "x": z[b, 1:1 + lx].copy()}
            out.append((instance, {"w": z[b, 1 + lx:].copy(), "e": e[b].copy()}, state["commit_t"][b]))
        return out

    def prove_batch(self, pairs, r):
        """prove() for a list of pairs in two enqueued phases (fold_begin, fold_end).  r: a (count, 4) array of challenges, or a callable
        that maps the list of commit_t to such an array -- the place of the caller's transcript.  Element b equals
        prove(*pairs[b], r[b]) in every word and flag."""
        state, commit_ts = self.fold_begin(pairs)
        return self.fold_end(state, r(commit_ts) if callable(r) else r)

    def check(self, u, x, w, e=None) -> tuple[int, int]:
        """(bad, first_bad) of kg_r1cs_check over z = (u | x | w): the rows i with (A z)_i (B z)_i != u (C z)_i + E_i and the first of
        them (m when there is none).  e: (m, 4) host array, a DeviceArray (e.g. a fold's output, still in flight on the context's
        stream), or None for E = 0."""
        z = self._z(u, x, w)
        de = None
        if e is not None:
            de = e if hasattr(e, "ptr") else self.ctx.upload(np.ascontiguousarray(e, dtype=np.uint64).reshape(-1, 4))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._dev]
        return self.ctx.r1cs_check(self.field, ptrs[0], ptrs[1], ptrs[2], self.m, z.ptr, u, de.ptr if de is not None else 0)

    def check_batch(self, pairs) -> np.ndarray:
        """check() for a list of (u, x, w, e) against the shape in ONE call (kg_r1cs_check_batch): the z vectors (u | x | w), the u and the E
        are uploaded as packed arrays.  e: (m, 4) host array or None (E = 0; when every e is None nothing is read).  Returns an array
        (count, 2) of (bad, first_bad) per pair, row b what check(*pairs[b]) returns."""
        pairs = list(pairs)
        count = len(pairs)
        if count == 0:
            return np.zeros((0, 2), dtype=np.uint32)
        el = lambda v: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
        z = np.ascontiguousarray(np.stack([np.concatenate([el(u), el(x), el(w)]) for u, x, w, _ in pairs]))
        du, dz, de = self.ctx.upload(np.stack([el(p[0])[0] for p in pairs])), self.ctx.upload(z), None
        if any(p[3] is not None for p in pairs):
            de = self.ctx.upload(np.stack([el(p[3]) if p[3] is not None else np.zeros((self.m, 4), dtype=np.uint64) for p in pairs]))
        ptrs = [tuple(d.ptr for d in trip) for trip in self._dev]
        return self.ctx.r1cs_check_batch(self.field, ptrs[0], ptrs[1], ptrs[2], self.m, dz.ptr, z.shape[1], count, du.ptr,
                                         de.ptr if de is not None else 0, self.m).numpy()

    def is_sat_relaxed(self, instance: dict, witness: dict) -> bool:
        """R1csShape::is_sat_relaxed (nova/src/relaxed_r1cs.rs:81-114) on the dicts prove() takes and returns: AZ o BZ = u CZ + E.
        Like the reference it leaves the commitments alone."""
        return self.check(instance["u"], instance["x"], witness["w"], witness["e"])[0] == 0

    def is_sat(self, instance: dict, witness: dict) -> bool:
        """R1csShape::is_sat (relaxed_r1cs.rs:117-146) for a fresh pair {"commit_w", "x"}, {"w"}: the constraints with u = 1, E = 0 and
        instance.commit_w == ck.commit(witness.w)"""
        if self.check(self._one(), instance["x"], witness["w"])[0] != 0:
            return False
        xy, inf = self.ck.commit(witness["w"])
        wxy, winf = instance["commit_w"]
        if bool(inf) or bool(winf):
            return bool(inf) == bool(winf)
        return bool((np.asarray(xy, dtype=np.uint64).reshape(-1) == np.asarray(wxy, dtype=np.uint64).reshape(-1)).all())

    def commit_t(self, u1, x1, w1, u2, x2, w2):
        """(T, commit_T): the cross term and ck.commit(&t) (prover.rs:33-35); T never leaves the device in between"""
        t = self.compute_cross_term_device(u1, x1, w1, u2, x2, w2)
        n = min(self.m, self.ck.len)
        xy, inf = self.ctx.commit(self.ck.cid, self.ck._g.ptr, self.ck._inf.ptr if self.ck._inf else 0, t.ptr, n)
        return t.numpy(), (xy, inf)


def groth16_setup(a, b, c, m: int, l: int, m_l_1: int, toxic, field_ops=None, ctx: Context | None = None) -> dict:
    """ZkSnark::setup (groth16/src/zksnark.rs:17-127) on the device through kg_groth16_setup_bn254, with the toxic waste injected
    (alpha, beta, gamma, delta, tau as rows of `toxic`; the reference draws them from its rng, :28-32).

    a, b, c: CSR triples (row_ptr, col, val) over z = x || w, host arrays.  Returns the Parameters dict `Prover` takes
    (device-computed, downloaded).  `field_ops` is accepted for callers of the round-3 signature and ignored: the five host-side
    scalars are computed behind the boundary now."""
    ctx = ctx or default_context()
    toxic = np.ascontiguousarray(toxic, dtype=np.uint64).reshape(5, 4)
    nv = l + m_l_1
    keep, mats = [], []
    for rp, col, val in (a, b, c):
        col = np.ascontiguousarray(col, dtype=np.uint64)
        val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
        d = [ctx.upload(np.ascontiguousarray(rp, dtype=np.uint64)), ctx.upload(col if len(col) else np.zeros(1, dtype=np.uint64)),
             ctx.upload(val if len(val) else np.zeros((1, 4), dtype=np.uint64))]
        keep.append(d)
        mats.append((d[0].ptr, d[1].ptr, d[2].ptr))
    lens = {"h": (max(m - 1, 0), 8), "l": (m_l_1, 8), "a": (nv, 8), "b_g1": (nv, 8), "b_g2": (nv, 16), "ic": (l, 8)}
    dev = {k: (ctx.empty((max(cnt, 1), w)), ctx.empty((max(cnt, 1),), dtype=np.uint8)) for k, (cnt, w) in lens.items()}
    crs = Groth16Crs()
    for k in ("h", "l", "a", "b_g1", "b_g2"):
        setattr(crs, "d_" + k, dev[k][0].ptr)
        setattr(crs, "d_" + k + "_inf", dev[k][1].ptr)
    gamma_g2, vk_inf = ctx.groth16_setup(mats[0], mats[1], mats[2], m, l, m_l_1, toxic, crs, dev["ic"][0].ptr, dev["ic"][1].ptr)
    P = {}
    for k, (cnt, w) in lens.items():
        P[k], P[k + "_inf"] = dev[k][0].numpy()[:cnt], dev[k][1].numpy()[:cnt]
    P["vk_g1"] = np.stack([np.array(crs.alpha_g1, dtype=np.uint64), np.array(crs.beta_g1, dtype=np.uint64), np.array(crs.delta_g1, dtype=np.uint64)])
    P["vk_g2"] = np.stack([np.array(crs.beta_g2, dtype=np.uint64), np.array(crs.delta_g2, dtype=np.uint64)])
    P["gamma_g2"] = gamma_g2
    P["delta_g1_inf"], P["delta_g2_inf"] = int(crs.delta_g1_inf), int(crs.delta_g2_inf)
    return P
