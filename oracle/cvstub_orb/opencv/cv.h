// Stand-in header (oracle/Makefile.ref, orb_ref_harness): everything lives in opencv2/core/core.hpp of this directory.
#include "../opencv2/core/core.hpp"
