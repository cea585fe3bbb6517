// nn_brute_terms.hip — nn_mfma_terms_kernel, the planned launch of the brute-force NN whose blocks
// also run their query block's terms pass, in a translation unit of its own: nn_brute.hip's device
// code compiled a third time with only that kernel and its launcher kept, and icp.hip's terms pass
// with it (why one kernel per unit: the note at the top of nn_brute.hip).
#define M3D_NN_BRUTE_TERMS_TU 1
#include "nn_brute.hip"
