// nn_brute_plan.hip — nn_mfma_plan_kernel, the planned (1-D) launch of the brute-force NN, in a
// translation unit of its own: nn_brute.hip's device code compiled again with only that kernel and
// its launcher kept (why: the note at the top of nn_brute.hip).
#define M3D_NN_BRUTE_PLAN_TU 1
#include "nn_brute.hip"
