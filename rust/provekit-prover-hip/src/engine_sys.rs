//! Hand-kept declarations of include/provekit_engine.h (libprovekit_engine.so): 15 functions, small enough to keep by hand;
//! `sys.rs` stays the generated image of provekit_hip.h alone.  tests/test_engine_host.py pins the header against the library.
#![allow(non_camel_case_types)]
use {
    crate::sys::{pk_r1cs, pk_whir_config},
    std::os::raw::{c_char, c_int, c_uint},
};

#[repr(C)]
pub struct pke_engine {
    _private: [u8; 0],
}
pub type pke_job = u64;

pub const PKE_MAX_LANES: c_uint = 32;
pub const PKE_AUTO_LANES_MAX: c_uint = 16;
pub const PKE_ERR_CANCELLED: c_int = -100;
pub const PKE_KEEP_HOST_WAIT: c_uint = 1;
pub const PKE_NO_JOB: pke_job = u64::MAX;

extern "C" {
    pub fn pke_engine_create(device: c_int, r1cs: *const pk_r1cs, num_constraints: usize, num_witnesses: usize, m: c_uint, m_0: c_uint, whir_witness: *const pk_whir_config, whir_for_hiding_spartan: *const pk_whir_config, lanes: c_uint, flags: c_uint, out: *mut *mut pke_engine) -> c_int;
    pub fn pke_create_error() -> *const c_char;
    pub fn pke_engine_destroy(engine: *mut pke_engine) -> c_int;
    pub fn pke_engine_lanes(engine: *const pke_engine) -> c_int;
    pub fn pke_engine_set_io_pattern(engine: *mut pke_engine, pattern: *const u8, n: usize) -> c_int;
    pub fn pke_engine_set_hash_version(engine: *mut pke_engine, version: c_int) -> c_int;
    pub fn pke_engine_set_witness_builders(engine: *mut pke_engine, postcard: *const u8, len: usize, n_witnesses: *mut usize, n_challenges: *mut usize, n_acir: *mut usize) -> c_int;
    pub fn pke_engine_domain_separator(engine: *const pke_engine, buf: *mut c_char, cap: usize, len: *mut usize) -> c_int;
    pub fn pke_submit(engine: *mut pke_engine, d_witness: *const u64, n_witness: usize, rng_seed32: *const u8, transcript_out: *mut u8, cap: usize, len: *mut usize, status: *mut c_int, job: *mut pke_job) -> c_int;
    pub fn pke_noir_submit(engine: *mut pke_engine, d_acir: *const u64, n_acir: usize, public_acir_idx: *const u32, n_public: usize, rng_seed32: *const u8, transcript_out: *mut u8, cap: usize, len: *mut usize, status: *mut c_int, job: *mut pke_job) -> c_int;
    pub fn pke_wait(engine: *mut pke_engine, job: pke_job) -> c_int;
    pub fn pke_wait_all(engine: *mut pke_engine) -> c_int;
    pub fn pke_prove_many(engine: *mut pke_engine, n: usize, d_witness: *const *const u64, n_witness: *const usize, rng_seed32: *const *const u8, transcript_out: *const *mut u8, cap: *const usize, len: *mut usize, status: *mut c_int, first_job: *mut pke_job) -> c_int;
    pub fn pke_noir_prove_many(engine: *mut pke_engine, n: usize, d_acir: *const *const u64, n_acir: *const usize, public_acir_idx: *const u32, n_public: usize, rng_seed32: *const *const u8, transcript_out: *const *mut u8, cap: *const usize, len: *mut usize, status: *mut c_int, first_job: *mut pke_job) -> c_int;
    pub fn pke_engine_last_error(engine: *const pke_engine, job: pke_job) -> *const c_char;
}
