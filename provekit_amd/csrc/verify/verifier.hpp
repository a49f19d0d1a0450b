// verifier.hpp -- what is behind a pkv_verifier: the statement (host core) and, once a context is attached, the device path's state
// (verify.hip owns it; the host part only knows how to ask for its release).
#pragma once
#include "core.hpp"

struct pkv_verifier {
    pkv::Statement st;
    std::string err;
    pk_ctx* ctx = nullptr;
    void* dev = nullptr;                      // verify.hip's DeviceState
    void (*dev_release)(pkv_verifier*) = nullptr;  // set by pkv_verifier_attach_device
};
