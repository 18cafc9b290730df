// tip_terrain_scaled.hip — tip_terrain.hip's reset and track kernels for wearers of different body sizes: the SCALED = true
// instantiations and their entries (include/tip_hip.h, "terrain": per-wearer body scale).  The kernels are tip_terrain.hip's templates,
// word for word; they are instantiated here, in a translation unit of their own, so that the unscaled ones compile exactly as they did
// alone.
#define TIP_TERRAIN_SCALED_TU
#include "tip_terrain.hip"

using namespace tip;

extern "C" {

int tip_terrain_reset_scaled(const void* skel, void* state, int n_slots, int grid_num, int max_regions, const int* slots, int count,
                             const float* s_init, const float* scale, tip_stream_t stream) {
    if (!skel || !state || !scale || ter_bad_shape(n_slots, grid_num, max_regions) || count < 0 || (count > 0 && !s_init)
        || reinterpret_cast<uintptr_t>(state) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL((terrain_reset_kernel<true, const float*>), dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<unsigned char*>(state), n_slots, grid_num, max_regions, slots, count,
                       s_init, scale);
    return tip_launch_status();
}

int tip_terrain_track_scaled(const void* skel, void* state, int n_slots, int grid_num, int max_regions, int diffuse_region, double grid_size,
                             const int* slots, const long long* begin, const long long* end, int count, long long n_rows,
                             const float* s_rest, const float* c_t, int nc, const unsigned char* valid, int flags, float* root_out,
                             float* viz_out, float* q_hist_out, int* fire_out, const float* scale, tip_stream_t stream) {
    if (!skel || !state || !scale || ter_bad_shape(n_slots, grid_num, max_regions) || count < 0 || tip_bad_rows(n_rows)
        || (nc != 8 && nc != 20) || reinterpret_cast<uintptr_t>(state) % 8 || diffuse_region < 1 || diffuse_region > tr::MAX_D
        || !(grid_size > 0.0) || !(grid_size < 1e6) || (flags & ~1) || ((flags & 1) && nc != 20))
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!begin || !end || !s_rest || !c_t || !root_out || !viz_out || !q_hist_out || !fire_out)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL((terrain_track_kernel<true, const float*>), dim3(count), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<unsigned char*>(state), n_slots, grid_num, max_regions, diffuse_region,
                       grid_size, slots, begin, end, n_rows, s_rest, c_t, nc, valid, flags, root_out, viz_out, q_hist_out, fire_out, scale);
    return tip_launch_status();
}

}  // extern "C"
