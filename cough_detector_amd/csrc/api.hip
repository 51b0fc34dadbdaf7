// Library-wide C-ABI entry points: version / arch / error text.
#include "common.h"

extern "C" int cough_amd_abi_version(void) { return COUGH_AMD_ABI_VERSION; }
extern "C" const char* cough_amd_arch(void) { return "gfx950"; }
COUGH_DEFINE_LAST_ERROR(cough_amd_last_error)
