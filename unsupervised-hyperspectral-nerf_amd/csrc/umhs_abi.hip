// The parts of libumhs_hip.so's C ABI that belong to no stage: error strings and the ABI version.
// Codes and version are defined in include/umhs_hip.h.
#include "umhs_common.h"

extern "C" const char* umhs_strerror(int code) {
  switch (code) {
    case UMHS_OK: return "ok";
    case UMHS_ERR_ARG: return "invalid argument";
    case UMHS_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels";
    case UMHS_ERR_WORKSPACE: return "workspace missing or too small";
    case UMHS_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
  }
}
extern "C" int umhs_abi_version(void) { return UMHS_ABI_VERSION; }
