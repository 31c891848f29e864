// The four-block (49 .. 64 features) instantiations of the persistent form of vaek_train_steps, in a translation unit of their own:
// see linear_moments_dev.h.
#include "linear_moments_dev.h"

namespace vaek {

LinPersistKernel lin_persist_four(int which) {
    return which == 0 ? lin_persist_kernel<4, 0, 0, 0, false> : lin_persist_kernel<4, 20, 20, 12, false>;
}
LinPersistGenKernel lin_persist_four_gen(int which) {
    return which == 0 ? lin_persist_kernel<4, 0, 0, 0, true> : lin_persist_kernel<4, 20, 20, 12, true>;
}
#ifdef VAEK_LIN_STAMPS
int lin_stamps_four(unsigned long long* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lin_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? 0 : -2;
}
#endif

}  // namespace vaek
