//! Many `WhirR1CSProver::prove` calls in flight from ONE caller thread (include/provekit_engine.h, libprovekit_engine.so).
//!
//! The reference gets this from rayon inside `prove`; [`crate::HipProver`] gives one thread one proof at a time.  The engine owns
//! K provers (context + scheme + arena each), one worker thread per lane and a job queue; `prove_many` blocks the caller until all
//! jobs are final.  A job's proof depends on (scheme, witness, randomness) only, never on the lane that ran it.
//!
//! Status: source only, like the rest of this crate -- it has not been compiled (no Rust toolchain where the library is built).
//! It is not wired into `lib.rs` and `build.rs` does not link the engine library, so the crate's existing users gain nothing they do
//! not call: to use it, add `pub mod engine; pub mod engine_sys;` to `lib.rs` and
//! `println!("cargo:rustc-link-lib=dylib=provekit_engine");` to `build.rs`, both behind one cargo feature.
use {
    crate::{engine_sys as esys, sys, whir_config_to_c, HipContext, HipR1CS},
    anyhow::{anyhow, ensure, Result},
    provekit_common::{FieldElement, WhirR1CSProof, WhirR1CSScheme, R1CS},
    std::{ffi::CStr, ptr},
};

/// `lanes` provers of `scheme` on the device of `ctx`.  `ctx` only uploads the R1CS and the witnesses; every lane has a context of
/// its own inside the engine.  `lanes == 0` lets the library pick (at most 16, by free device memory).
pub struct HipProofEngine<'a> {
    ctx: &'a HipContext,
    r1cs: HipR1CS<'a>, // dropped after `raw` (see Drop): a pk_r1cs outlives the schemes bound to it
    raw: *mut esys::pke_engine,
}

impl<'a> HipProofEngine<'a> {
    pub fn new(ctx: &'a HipContext, device: i32, scheme: &WhirR1CSScheme, r1cs: &R1CS, lanes: u32) -> Result<Self> {
        ensure!(lanes <= esys::PKE_MAX_LANES, "at most {} lanes", esys::PKE_MAX_LANES);
        let dev = HipR1CS::upload(ctx, r1cs)?;
        let (w, b) = (whir_config_to_c(&scheme.whir_witness)?, whir_config_to_c(&scheme.whir_for_hiding_spartan)?);
        let mut raw = ptr::null_mut();
        let rc = unsafe {
            esys::pke_engine_create(device, dev.raw, dev.num_constraints, dev.num_witnesses, scheme.m as _, scheme.m_0 as _, &w, &b, lanes, 0, &mut raw)
        };
        if rc != sys::PK_OK {
            let why = unsafe { CStr::from_ptr(esys::pke_create_error()) }.to_string_lossy().into_owned();
            return Err(anyhow!("libprovekit_engine status {rc}: {why}"));
        }
        let this = Self { ctx, r1cs: dev, raw };
        // the reference's own IO pattern on every lane, refused unless it declares pk_prove's operations (as HipProver::new)
        let io = scheme.create_io_pattern();
        let bytes = io.as_bytes();
        let rc = unsafe { esys::pke_engine_set_io_pattern(this.raw, bytes.as_ptr(), bytes.len()) };
        if rc != sys::PK_OK {
            return Err(anyhow!("libprovekit_engine status {rc}: {}", this.error(esys::PKE_NO_JOB)));
        }
        Ok(this)
    }

    pub fn lanes(&self) -> usize {
        unsafe { esys::pke_engine_lanes(self.raw) as usize }
    }

    fn error(&self, job: esys::pke_job) -> String {
        unsafe { CStr::from_ptr(esys::pke_engine_last_error(self.raw, job)) }.to_string_lossy().into_owned()
    }

    /// One proof per witness, in order; fresh OS randomness per proof (NULL seeds), as the reference's thread_rng.  A failed job
    /// does not stop the others: every entry is that job's own `Result`.
    pub fn prove_many(&self, witnesses: &[Vec<FieldElement>]) -> Result<Vec<Result<WhirR1CSProof>>> {
        let n = witnesses.len();
        for w in witnesses {
            ensure!(w.len() == self.r1cs.num_witnesses, "Unexpected witness length for R1CS instance"); // whir_r1cs.rs:43-46
        }
        let d_z = witnesses.iter().map(|w| self.ctx.upload(w)).collect::<Result<Vec<_>>>()?;
        let d_ptr: Vec<*const u64> = d_z.iter().map(|d| d.ptr as *const u64).collect();
        let n_w: Vec<usize> = d_z.iter().map(|d| d.len).collect();
        let mut bufs: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; 4 << 20]).collect();
        let out: Vec<*mut u8> = bufs.iter_mut().map(|b| b.as_mut_ptr()).collect();
        let cap: Vec<usize> = bufs.iter().map(|b| b.len()).collect();
        let (mut len, mut status, mut first) = (vec![0usize; n], vec![0i32; n], 0u64);
        // the call's own return repeats the first failed job's status: the per-job slots say everything
        let _ = unsafe {
            esys::pke_prove_many(self.raw, n, d_ptr.as_ptr(), n_w.as_ptr(), ptr::null(), out.as_ptr(), cap.as_ptr(), len.as_mut_ptr(), status.as_mut_ptr(), &mut first)
        };
        Ok(bufs
            .into_iter()
            .enumerate()
            .map(|(i, mut transcript)| {
                if status[i] != sys::PK_OK {
                    return Err(anyhow!("libprovekit_hip status {}: {}", status[i], self.error(first + i as u64)));
                }
                transcript.truncate(len[i]);
                Ok(WhirR1CSProof { transcript })
            })
            .collect())
    }
}

impl Drop for HipProofEngine<'_> {
    fn drop(&mut self) {
        unsafe { esys::pke_engine_destroy(self.raw) }; // the lanes' schemes go first; the R1CS field drops after this body
    }
}
