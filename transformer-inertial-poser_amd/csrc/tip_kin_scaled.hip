// tip_kin_scaled.hip — tip_kin.hip's FK, reset and track kernels for wearers of different body sizes: the SCALED = true instantiations
// and their entries (include/tip_hip.h, "kinematics": per-wearer body scale).  The kernels are tip_kin.hip's templates, word for word;
// they are instantiated here, in a translation unit of their own, so that the unscaled ones compile exactly as they did alone.
#define TIP_KIN_SCALED_TU
#include "tip_kin.hip"

using namespace tip;

extern "C" {

int tip_kin_fk_scaled(const void* skel, const float* q, int ldq, long long n, float* pq_g, float* pq_jf, const float* scale,
                      tip_stream_t stream) {
    if (!skel || !q || !pq_g || !scale || tip_bad_rows(n) || ldq < kn::NQ) return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_fk_kernel<true, const float*>), dim3((unsigned)((n + kn::LANES - 1) / kn::LANES)), dim3(kn::LANES), 0,
                       static_cast<hipStream_t>(stream), static_cast<const KinSkel*>(skel), q, ldq, n, pq_g, pq_jf, scale);
    return tip_launch_status();
}

int tip_kin_track_reset_scaled(const void* skel, void* carry, int n_slots, const int* slots, int count, const float* s_init,
                               const float* scale, tip_stream_t stream) {
    if (!skel || !carry || !scale || tip_bad_count(n_slots) || count < 0 || (count > 0 && !s_init)
        || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_reset_kernel<true, const float*>), dim3((count + kn::LANES - 1) / kn::LANES), dim3(kn::LANES), 0,
                       static_cast<hipStream_t>(stream), static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots,
                       count, s_init, scale);
    return tip_launch_status();
}

int tip_kin_track_scaled(const void* skel, void* carry, int n_slots, const int* slots, const long long* begin, const long long* end,
                         int count, long long n_rows, const float* s_rest, const float* c_t, int nc, const unsigned char* valid,
                         float* root_out, float* viz_out, const float* scale, tip_stream_t stream) {
    if (!skel || !carry || !scale || tip_bad_count(n_slots) || count < 0 || tip_bad_rows(n_rows) || (nc != 8 && nc != 20)
        || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!begin || !end || !s_rest || !c_t || !root_out || !viz_out)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_track_kernel<true, const float*>), dim3(count), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots, begin, end, n_rows, s_rest, c_t,
                       nc, valid, root_out, viz_out, scale);
    return tip_launch_status();
}

}  // extern "C"
