//! Glue between Kogarashi's own types (zkstd traits, bn-254, grumpkin) and the MI355X backend's C ABI.
//!
//! The reference reaches its hot path through crate-internal generic functions:
//!   `groth16/src/msm.rs:6`          `msm_curve_addition<C: BNAffine>(bases, coeffs) -> C::Extended`
//!   `groth16/src/fft.rs:92-154`     `Fft::<F>::{dft, idft, coset_dft, coset_idft, divide_by_z_on_coset}`
//!   `nova/src/pedersen.rs:15`       `PedersenCommitment::<C>::commit(&self, m) -> C`
//!   `groth16/src/prover.rs:20`      `Prover::create_proof`
//!   `nova/src/prover.rs:53`         `Prover::compute_cross_term`
//! The patches in `rust/patches/` add one `#[cfg(feature = "gpu")]` early return to each of them that calls the
//! generic entry points below.  They dispatch on `TypeId` (the `'static` bound comes from the one-line patch to
//! `zkstd::traits::Group`), so the reference's generic signatures stay as they are; a type the backend does not
//! serve (or any non-zero status) yields `None` and the crate's own CPU body runs -- the *library* has no CPU path.
//!
//! Marshalling: field elements are passed as they lie in memory (`Fr(pub [u64; 4])`, `Fq`, made
//! `#[repr(transparent)]` by `patches/bn254.diff`); points are `repr(Rust)` structs and are marshalled explicitly
//! through `get_x() / get_y() / is_identity()` into `x | y` words plus a flag byte.
use core::any::TypeId;
use core::ffi::c_void;
use core::ptr;
use std::collections::HashMap;
use std::sync::Mutex;

use bn_254::{Fq, Fq2, Fr, G1Affine, G1Projective, G2Affine, G2Projective};
use grumpkin::{Affine as GkAffine, Projective as GkProjective};
use kogarashi_amd_sys as sys;
use zkstd::common::{BNAffine, BNProjective, CurveGroup, Group};

mod csr;
pub mod fft;
pub mod groth16;
pub mod nova;
pub mod pedersen;

/// A backend failure; callers in the patched crates treat it as "use the CPU body".
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Status(pub i32);

fn check(rc: i32) -> Result<(), Status> {
    if rc == sys::KG_OK {
        Ok(())
    } else {
        Err(Status(rc))
    }
}

/// One `kg_ctx` (a GPU, its streams, twiddle caches and MSM work space).  `Send`: the reference's types are
/// `Send + Sync` and the ABI allows any thread; calls on one context are serialised by `&mut self` / the mutex below.
pub struct Context {
    raw: *mut sys::KgCtx,
}
unsafe impl Send for Context {}

impl Context {
    pub fn new(device: i32) -> Result<Self, Status> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::kg_ctx_create(device, &mut raw) })?;
        Ok(Self { raw })
    }
    pub fn raw(&self) -> *mut sys::KgCtx {
        self.raw
    }
    pub fn device_count() -> i32 {
        unsafe { sys::kg_device_count() }
    }
}
impl Drop for Context {
    fn drop(&mut self) {
        unsafe { sys::kg_ctx_destroy(self.raw) }
    }
}

/// Device memory owned through the ABI's own allocator (a Rust host never links the HIP runtime).
pub struct DeviceBuf {
    ctx: *mut sys::KgCtx,
    ptr: *mut c_void,
    bytes: usize,
}
impl DeviceBuf {
    pub fn new(ctx: &Context, bytes: usize) -> Result<Self, Status> {
        let mut p = ptr::null_mut();
        check(unsafe { sys::kg_malloc(ctx.raw, bytes.max(1), &mut p) })?;
        Ok(Self { ctx: ctx.raw, ptr: p, bytes })
    }
    pub fn from_words(ctx: &Context, w: &[u64]) -> Result<Self, Status> {
        let b = Self::new(ctx, w.len() * 8)?;
        check(unsafe { sys::kg_memcpy_h2d(ctx.raw, b.ptr, w.as_ptr() as *const c_void, w.len() * 8) })?;
        Ok(b)
    }
    pub fn from_bytes(ctx: &Context, w: &[u8]) -> Result<Self, Status> {
        let b = Self::new(ctx, w.len())?;
        check(unsafe { sys::kg_memcpy_h2d(ctx.raw, b.ptr, w.as_ptr() as *const c_void, w.len()) })?;
        Ok(b)
    }
    pub fn read_words(&self, out: &mut [u64]) -> Result<(), Status> {
        debug_assert!(out.len() * 8 <= self.bytes);
        check(unsafe { sys::kg_memcpy_d2h(self.ctx, out.as_mut_ptr() as *mut c_void, self.ptr, out.len() * 8) })
    }
    pub fn as_u64(&self) -> *mut u64 {
        self.ptr as *mut u64
    }
    pub fn as_u8(&self) -> *mut u8 {
        self.ptr as *mut u8
    }
}
impl Drop for DeviceBuf {
    fn drop(&mut self) {
        unsafe { sys::kg_free(self.ctx, self.ptr) };
    }
}

mod global {
    use super::*;
    use std::sync::{Arc, MutexGuard};

    /// One GPU's context behind its OWN lock: threads that work on different GPUs (or wait for different calls) do not
    /// serialise on a process-wide guard -- the reference's callers fan out on the rayon pool ("callable from any
    /// thread, re-entrant").  Calls on one context are serialised, as the ABI asks.
    pub struct CtxSlot(Mutex<Context>);

    // `Mutex::new` is const on the reference's pinned toolchain (nightly-2022-11-14); `OnceLock` is not stable there.
    // None: not probed yet; Some(vec): probed -- an empty vec means "no device", and is never probed again.  This lock is held
    // only while the list is created or its `Arc` is cloned, never across a backend call.
    static CTXS: Mutex<Option<Arc<Vec<CtxSlot>>>> = Mutex::new(None);
    // round-robin cursor of `lock_any`
    static NEXT: Mutex<Option<usize>> = Mutex::new(None);

    /// The contexts of the visible GPUs (one each).  Cheap to obtain and to hold: a reference-counted list, no lock.
    #[derive(Clone)]
    pub struct Contexts(Arc<Vec<CtxSlot>>);
    impl Contexts {
        pub fn len(&self) -> usize {
            self.0.len()
        }
        /// context i, for calls tied to state resident on that GPU (a CRS, a shape)
        pub fn lock(&self, i: usize) -> Option<MutexGuard<'_, Context>> {
            self.0.get(i)?.0.lock().ok()
        }
        /// any context, for calls that bring their inputs along (a transform, an MSM over host slices): the first one that is
        /// free, starting at a round-robin cursor; the cursor's own context if all are busy
        pub fn lock_any(&self) -> Option<MutexGuard<'_, Context>> {
            let n = self.0.len();
            let start = {
                let mut c = NEXT.lock().ok()?;
                let v = c.unwrap_or(0);
                *c = Some((v + 1) % n.max(1));
                v % n.max(1)
            };
            for k in 0..n {
                if let Ok(g) = self.0[(start + k) % n].0.try_lock() {
                    return Some(g);
                }
            }
            self.0.get(start)?.0.lock().ok()
        }
        /// the contexts `idx` names (duplicates allowed), locked in ascending index order (one order everywhere: no deadlock);
        /// the result holds one guard per DISTINCT index, sorted -- `position(i)` finds a context's guard.  For calls that
        /// span a few GPUs (`kg_groth16_prove_sharded` over three) without stopping the node's other callers.
        pub fn lock_set(&self, idx: &[usize]) -> Option<(Vec<usize>, Vec<MutexGuard<'_, Context>>)> {
            let mut order: Vec<usize> = idx.to_vec();
            order.sort_unstable();
            order.dedup();
            let mut v = Vec::with_capacity(order.len());
            for &i in order.iter() {
                v.push(self.0.get(i)?.0.lock().ok()?);
            }
            Some((order, v))
        }
        /// every context, in index order (one order everywhere: no deadlock), for the calls that span the node
        /// (`kg_sharded_key_*`, `kg_groth16_prove_sharded`)
        pub fn lock_all(&self) -> Option<Vec<MutexGuard<'_, Context>>> {
            let mut v = Vec::with_capacity(self.0.len());
            for s in self.0.iter() {
                v.push(s.0.lock().ok()?);
            }
            Some(v)
        }
    }

    /// One context per visible GPU, created on first use; `None` when no device is present (CPU bodies run).
    pub fn contexts() -> Option<Contexts> {
        let mut guard = CTXS.lock().ok()?;
        if guard.is_none() {
            let mut v = Vec::new();
            // kept for the ABI: kg_init sets nothing (the hardware queue count is the machine's setting).
            unsafe { sys::kg_init() };
            let n = Context::device_count();
            for d in 0..n.max(0) {
                match Context::new(d) {
                    Ok(c) => v.push(CtxSlot(Mutex::new(c))),
                    Err(_) => {
                        v.clear();
                        break;
                    }
                }
            }
            *guard = Some(Arc::new(v));
        }
        let list = guard.as_ref()?.clone();
        if list.is_empty() {
            return None;
        }
        Some(Contexts(list))
    }
}
pub use global::{contexts, Contexts};

// ---- TypeId casts (same type on both sides, so these are identity conversions) ------------------------------------
pub(crate) fn same<A: 'static, B: 'static>() -> bool {
    TypeId::of::<A>() == TypeId::of::<B>()
}
pub(crate) fn cast_slice<A: 'static, B: 'static>(s: &[A]) -> Option<&[B]> {
    if same::<A, B>() {
        Some(unsafe { &*(s as *const [A] as *const [B]) })
    } else {
        None
    }
}
pub(crate) fn cast_val<A: 'static + Copy, B: 'static + Copy>(a: A) -> Option<B> {
    if same::<A, B>() {
        Some(unsafe { *(&a as *const A as *const B) })
    } else {
        None
    }
}

/// `&[Fr]` / `&[Fq]` as the ABI's n x 4 words (the structs are `repr(transparent)` over `[u64; 4]`).
pub(crate) fn scalar_words<S: 'static>(s: &[S]) -> Option<(*const u64, i32)> {
    const _: () = assert!(core::mem::size_of::<Fr>() == 32 && core::mem::size_of::<Fq>() == 32);
    if same::<S, Fr>() {
        Some((s.as_ptr() as *const u64, sys::KG_FR))
    } else if same::<S, Fq>() {
        Some((s.as_ptr() as *const u64, sys::KG_FQ))
    } else {
        None
    }
}

/// The three curves of the path, with their ABI marshalling.
pub trait GpuCurve: BNAffine + Copy + 'static {
    const CURVE: i32;
    /// u64 words of one affine point (x | y)
    const WORDS: usize;
    fn put_xy(&self, out: &mut Vec<u64>);
    fn affine_from(words: &[u64], inf: bool) -> Self;
    /// ABI projective output (x, y, z) with z in {0, 1}
    fn extended_from(words: &[u64]) -> Self::Extended;
}

fn fq(w: &[u64]) -> Fq {
    Fq::new_unchecked([w[0], w[1], w[2], w[3]])
}
fn fr(w: &[u64]) -> Fr {
    Fr::new_unchecked([w[0], w[1], w[2], w[3]])
}
fn fq2(w: &[u64]) -> Fq2 {
    Fq2::new_unchecked([fq(&w[0..4]), fq(&w[4..8])])
}

impl GpuCurve for G1Affine {
    const CURVE: i32 = sys::KG_G1;
    const WORDS: usize = 8;
    fn put_xy(&self, out: &mut Vec<u64>) {
        out.extend_from_slice(self.get_x().inner());
        out.extend_from_slice(self.get_y().inner());
    }
    fn affine_from(w: &[u64], inf: bool) -> Self {
        if inf {
            G1Affine::ADDITIVE_IDENTITY
        } else {
            G1Affine::from_x_and_y(fq(&w[0..4]), fq(&w[4..8]))
        }
    }
    fn extended_from(w: &[u64]) -> G1Projective {
        G1Projective::new_unchecked(fq(&w[0..4]), fq(&w[4..8]), fq(&w[8..12]))
    }
}
impl GpuCurve for GkAffine {
    const CURVE: i32 = sys::KG_GRUMPKIN;
    const WORDS: usize = 8;
    fn put_xy(&self, out: &mut Vec<u64>) {
        out.extend_from_slice(self.get_x().inner());
        out.extend_from_slice(self.get_y().inner());
    }
    fn affine_from(w: &[u64], inf: bool) -> Self {
        if inf {
            GkAffine::ADDITIVE_IDENTITY
        } else {
            GkAffine::from_x_and_y(fr(&w[0..4]), fr(&w[4..8]))
        }
    }
    fn extended_from(w: &[u64]) -> GkProjective {
        GkProjective::new_unchecked(fr(&w[0..4]), fr(&w[4..8]), fr(&w[8..12]))
    }
}
impl GpuCurve for G2Affine {
    const CURVE: i32 = sys::KG_G2;
    const WORDS: usize = 16;
    fn put_xy(&self, out: &mut Vec<u64>) {
        let (x, y) = (self.get_x(), self.get_y());
        for c in x.inner().iter().chain(y.inner().iter()) {
            out.extend_from_slice(c.inner()); // Fq2::inner: patches/bn254.diff
        }
    }
    fn affine_from(w: &[u64], inf: bool) -> Self {
        if inf {
            G2Affine::ADDITIVE_IDENTITY
        } else {
            G2Affine::from_x_and_y(fq2(&w[0..8]), fq2(&w[8..16]))
        }
    }
    fn extended_from(w: &[u64]) -> G2Projective {
        G2Projective::new_unchecked(fq2(&w[0..8]), fq2(&w[8..16]), fq2(&w[16..24]))
    }
}

/// x | y words and flag bytes of a point slice
pub(crate) fn marshal<C: GpuCurve>(pts: &[C]) -> (Vec<u64>, Vec<u8>) {
    let mut xy = Vec::with_capacity(pts.len() * C::WORDS);
    let mut inf = Vec::with_capacity(pts.len());
    for p in pts {
        p.put_xy(&mut xy);
        inf.push(p.is_identity() as u8);
    }
    (xy, inf)
}

/// How `msm` treats the base slice of a call (`KOGARASHI_AMD_MSM_RESIDENT`, read once):
///   unset / `hash`   keep the slice resident on GPU 0 in the MSM's internal form (`kg_bases_register`), keyed by address, length and
///                    curve, and re-validate it on EVERY call with a digest of EVERY point (all coordinate words and the identity flag):
///                    exact -- `msm_curve_addition(&[C], ...)` borrows a slice and promises nothing about its content between calls
///                    (`groth16/src/msm.rs:6`), so a base rewritten in place is seen whichever index it has.  The digest is O(n) host
///                    work, about 2.5 ms per 2^20 G1 points (one pass over 64 MiB), in front of a 1.6 ms MSM -- the price of keeping
///                    a borrowed slice resident without a promise; a host that can make the promise uses `register_bases` (no digest
///                    at all) or `sampled`.
///   `sampled`        the same cache validated with a digest of up to 256 evenly spaced points (~10 us): for hosts whose base slices are
///                    immutable in practice (CRS vectors, commitment keys: `groth16/src/params.rs:6-28`, `nova/src/pedersen.rs:6-13`).
///                    A base rewritten in place at an index the sample misses goes UNSEEN -- opt in only with that promise.
///   `0`              nothing is kept: every call marshals and uploads its bases (`kg_msm_host`).
/// `register_bases` / `ResidentMsmBases::msm` is the explicit alternative: the caller owns the handle and the promise.
#[derive(Clone, Copy, PartialEq, Eq)]
enum ResidencyMode {
    Off,
    Probe,
    Hash,
}
fn residency_mode() -> ResidencyMode {
    static MODE: Mutex<Option<ResidencyMode>> = Mutex::new(None);
    let mut m = match MODE.lock() {
        Ok(m) => m,
        Err(_) => return ResidencyMode::Off,
    };
    *m.get_or_insert_with(|| match std::env::var("KOGARASHI_AMD_MSM_RESIDENT").ok().as_deref() {
        Some("0") | Some("off") => ResidencyMode::Off,
        Some("sampled") | Some("probe") => ResidencyMode::Probe,
        _ => ResidencyMode::Hash,
    })
}

/// 128-bit digest of the points at `step`-spaced indices (always including the last one): every coordinate word and the flag.
/// `step` = 1 is the full content hash.  Not cryptographic: it guards a cache against stale content, not against an adversary.
fn digest<C: GpuCurve>(pts: &[C], step: usize) -> [u64; 2] {
    let (mut h1, mut h2) = (0xcbf2_9ce4_8422_2325u64, 0x9e37_79b9_7f4a_7c15u64);
    let mut words = Vec::with_capacity(C::WORDS);
    let mut take = |i: usize, h1: &mut u64, h2: &mut u64| {
        words.clear();
        pts[i].put_xy(&mut words);
        let flag = pts[i].is_identity() as u64;
        for &w in words.iter().chain(core::iter::once(&(flag ^ (i as u64).rotate_left(17)))) {
            *h1 = (*h1 ^ w).wrapping_mul(0x0000_0100_0000_01b3);
            *h2 = (h2.rotate_left(23) ^ w).wrapping_mul(0xff51_afd7_ed55_8ccd).wrapping_add(0x2545_f491_4f6c_dd1d);
        }
    };
    let n = pts.len();
    let mut i = 0;
    while i < n {
        take(i, &mut h1, &mut h2);
        i += step.max(1);
    }
    if n > 0 {
        take(n - 1, &mut h1, &mut h2);
    }
    [h1, h2 ^ n as u64]
}
const PROBE_POINTS: usize = 256;
fn digest_for<C: GpuCurve>(pts: &[C], mode: ResidencyMode) -> [u64; 2] {
    let step = if mode == ResidencyMode::Hash { 1 } else { (pts.len() / PROBE_POINTS).max(1) };
    digest(pts, step)
}

/// A base slice resident on GPU 0 in the MSM's internal form (`kg_bases_register`).  Dropping its buffers releases the
/// registration too (`kg_free` unregisters the array it frees); whoever drops it holds GPU 0's lock.
struct Resident {
    xy: DeviceBuf,
    inf: Option<DeviceBuf>,
    n: usize,
    curve: i32,
    digest: [u64; 2],
    stamp: u64,
}
unsafe impl Send for Resident {}
impl Resident {
    fn upload<C: GpuCurve>(ctx: &Context, bases: &[C], digest: [u64; 2]) -> Option<Self> {
        let (xy, inf) = marshal(bases);
        let d_xy = DeviceBuf::from_words(ctx, &xy).ok()?;
        let d_inf = if inf.iter().any(|&f| f != 0) { Some(DeviceBuf::from_bytes(ctx, &inf).ok()?) } else { None };
        let pi = d_inf.as_ref().map(|d| d.as_u8() as *const u8).unwrap_or(ptr::null());
        let rc = unsafe { sys::kg_bases_register(ctx.raw(), C::CURVE, d_xy.as_u64() as *const u64, pi, bases.len()) };
        if rc != sys::KG_OK {
            return None;
        }
        Some(Self { xy: d_xy, inf: d_inf, n: bases.len(), curve: C::CURVE, digest, stamp: 0 })
    }
    /// sum_i coeffs[i] * bases[i] over `n <= len` pairs: the scalars go up in index slices under the accumulations
    /// (`kg_msm_host_scalars`), nothing else crosses the bus
    fn run(&self, ctx: &Context, coeffs: *const u64, n: usize) -> Option<[u64; 24]> {
        let pi = self.inf.as_ref().map(|d| d.as_u8() as *const u8).unwrap_or(ptr::null());
        let mut out = [0u64; 24];
        let rc = unsafe { sys::kg_msm_host_scalars(ctx.raw(), self.curve, self.xy.as_u64() as *const u64, pi, coeffs, n.min(self.n), out.as_mut_ptr()) };
        if rc == sys::KG_OK { Some(out) } else { None }
    }
}

/// Explicit residency: the handle `register_bases` returns.  The caller keeps the slice's content unchanged while the handle
/// lives (the handle does not look at the slice again); dropping it releases the device copy.
pub struct ResidentMsmBases(Option<Resident>);
impl ResidentMsmBases {
    /// `msm_curve_addition(bases, coeffs)` against the registered slice (zip semantics, msm.rs:25)
    pub fn msm<C: GpuCurve>(&self, coeffs: &[C::Scalar]) -> Option<C::Extended>
    where
        C::Scalar: 'static,
    {
        let r = self.0.as_ref()?;
        if C::CURVE != r.curve {
            return None;
        }
        let (sw, _) = scalar_words(coeffs)?;
        let ctxs = contexts()?;
        let ctx = ctxs.lock(0)?;
        Some(C::extended_from(&r.run(&ctx, sw, coeffs.len())?))
    }
}
impl Drop for ResidentMsmBases {
    fn drop(&mut self) {
        // the buffers are freed (and the registration dropped) under GPU 0's lock: calls on one context are serialised
        let ctxs = contexts();
        let _held = ctxs.as_ref().and_then(|c| c.lock(0));
        self.0.take();
    }
}

/// Upload and convert `bases` once; the handle's `msm` then moves only scalars.
pub fn register_bases<C: GpuCurve>(bases: &[C]) -> Option<ResidentMsmBases> {
    if bases.is_empty() {
        return None;
    }
    let ctxs = contexts()?;
    let ctx = ctxs.lock(0)?;
    Some(ResidentMsmBases(Some(Resident::upload(&ctx, bases, digest(bases, 1))?)))
}

/// `is_on_curve` over a whole slice (group.rs:59-65) and, with `subgroup`, `[r]P = O` for G2 (the call site of
/// `G2Affine::is_torsion_free`, bn254/src/g2.rs:26): `kg_points_check` on an uploaded copy.  Returns (number of invalid points, index
/// of the first one or `points.len()`); `None` when the backend is unavailable.  What a host runs on deserialised `Parameters` or a
/// commitment key before `register_bases`.
pub fn points_check<C: GpuCurve>(points: &[C], subgroup: bool) -> Option<(usize, usize)> {
    if points.is_empty() {
        return Some((0, 0));
    }
    let ctxs = contexts()?;
    let ctx = ctxs.lock(0)?;
    let (xy, inf) = marshal(points);
    let d_xy = DeviceBuf::from_words(&ctx, &xy).ok()?;
    let d_inf = DeviceBuf::from_bytes(&ctx, &inf).ok()?;
    let checks = sys::KG_CHECK_CURVE | if subgroup { sys::KG_CHECK_SUBGROUP } else { 0 };
    let (mut bad, mut first) = (0usize, 0usize);
    let rc = unsafe { sys::kg_points_check(ctx.raw(), C::CURVE, d_xy.as_u64() as *const u64, d_inf.as_u8() as *const u8, points.len(), checks, ptr::null_mut(), &mut bad, &mut first) };
    if rc == sys::KG_OK { Some((bad, first)) } else { None }
}

const MSM_CACHE_SLOTS: usize = 8;
static MSM_BASES: Mutex<Option<(u64, HashMap<(usize, usize, i32), Resident>)>> = Mutex::new(None);

fn msm_typed<C: GpuCurve>(bases: &[C], coeffs: *const u64, n: usize) -> Option<C::Extended> {
    if n == 0 {
        return None;                                           // the CPU body returns the identity at once
    }
    let ctxs = contexts()?;
    let bases = &bases[..n];
    let mode = residency_mode();
    if n < (1 << 14) || mode == ResidencyMode::Off {
        // small calls (the prover's `inputs` MSMs of length l), or a host that keeps nothing resident: one host-array call
        let ctx = ctxs.lock_any()?;
        let (xy, inf) = marshal(bases);
        let mut out = [0u64; 24];
        let rc = unsafe { sys::kg_msm_host(ctx.raw(), C::CURVE, xy.as_ptr(), inf.as_ptr(), coeffs, n, out.as_mut_ptr()) };
        return if rc == sys::KG_OK { Some(C::extended_from(&out)) } else { None };
    }
    // Marshalling 2^20 `repr(Rust)` points through `get_x() / get_y()` costs tens of milliseconds and the upload 1.3 ms (64 MB over
    // PCIe) around a 1.6 ms device MSM: both are paid once per slice.  A call then validates the slice (sampled digest: ~10 us; full
    // digest under KOGARASHI_AMD_MSM_RESIDENT=hash: a few ms) and uploads its scalars inside `kg_msm_host_scalars`.
    let print = digest_for(bases, mode);
    let ctx = ctxs.lock(0)?;                                   // the cache lives on GPU 0
    let mut lock = MSM_BASES.lock().ok()?;
    let (clock, cache) = lock.get_or_insert_with(|| (0, HashMap::new()));
    *clock += 1;
    let id = (bases.as_ptr() as usize, n, C::CURVE);
    if cache.get(&id).map(|r| r.digest != print).unwrap_or(false) {
        cache.remove(&id);                                     // stale: freed (and unregistered) here, under GPU 0's lock
    }
    if !cache.contains_key(&id) {
        if cache.len() >= MSM_CACHE_SLOTS {                    // evict the least recently used slice
            let oldest = cache.iter().min_by_key(|(_, r)| r.stamp).map(|(k, _)| *k)?;
            cache.remove(&oldest);
        }
        cache.insert(id, Resident::upload(&ctx, bases, print)?);
    }
    let r = cache.get_mut(&id)?;
    r.stamp = *clock;
    Some(C::extended_from(&r.run(&ctx, coeffs, n)?))
}

/// `groth16::msm::msm_curve_addition` on the device: sum over `min(len)` pairs (the reference zips, msm.rs:25).
/// Returns `(x, y, 1)` / `(0, 1, 0)`; equal to the CPU result under the crate's projective `PartialEq`
/// (cross-multiplication, macros/curve/weierstrass/group.rs:89-97) and bit for bit after `.into()`.
pub fn msm<C: BNAffine + 'static>(bases: &[C], coeffs: &[C::Scalar]) -> Option<C::Extended>
where
    C::Scalar: 'static,
    C::Extended: 'static + Copy,
{
    let n = bases.len().min(coeffs.len());
    let (sw, _) = scalar_words(coeffs)?;
    if let Some(b) = cast_slice::<C, G1Affine>(bases) {
        return cast_val(msm_typed(b, sw, n)?);
    }
    if let Some(b) = cast_slice::<C, G2Affine>(bases) {
        return cast_val(msm_typed(b, sw, n)?);
    }
    if let Some(b) = cast_slice::<C, GkAffine>(bases) {
        return cast_val(msm_typed(b, sw, n)?);
    }
    None
}
