// tip_sensor.hip — the sensor front end: raw IMU packets and the per-slot calibration, in front of the streaming engines' `raw`
// buffer.  The reference does this arithmetic on the host between its socket reader and RTRunner.step (live_demo_new.py):
//
//   :97-112            a packet is 6 sensors x (quaternion, sensor-frame acceleration), 42 floats -> 6 rotation matrices (Q2R) +
//                      6 accelerations
//   :150-158, :221-226 heading reset: the mean of the readings over a hold gives R_Gn_Gp (the mean matrices AS THEY ARE: the demo
//                      does not re-orthonormalise, neither does this file) and acc_offset_Gp
//   :243-248, :52-62   T-pose: a second mean gives R_Gn_S0, and R_B0_S0 = R_Gp_B0^T (R_Gn_Gp^T R_Gn_S0)
//   :161-175           per frame: R_Gp_St = R_Gn_Gp^T R_Gn_St, R_Gp_Bt = R_Gp_St R_B0_S0^T, acc_Gp = clip(R_Gp_St acc - acc_offset,
//                      +-MAX_ACC); the 72-column frame is the 54 rotation columns, then the 18 acceleration columns
//
// Q2R is fairmotion's, which is scipy's Rotation.from_quat(q).as_matrix(): q = (x, y, z, w), normalised first.
//
// One calibration block per slot (SensorCal) in a caller-owned device buffer, as the stream state.  The block, Q2R and the per-sensor
// body of the transform (sensor_row) live in tip_sensor.h, which tip_fill.hip includes too.  Kernels:
//
//   sensor_transform_kernel    the per-frame hot path: one thread per (slot, sensor), fp32, writes the slot's 9 + 3 columns of raw
//   sensor_accumulate_kernel   one thread per (slot, sensor): a slot in phase 1 or 3 adds its Q2R matrices (fp64 from the fp32
//                              quaternion) and raw accelerations to the fp64 sums; any other slot is not written at all
//   sensor_begin_kernel        listed slots: sums and count to zero, phase 0 | 2 | 4 -> 1 (heading) or 2 -> 3 (T-pose)
//   sensor_finish_kernel       listed slots: phase 1 -> 2 (R_Gn_Gp, acc_offset = the means), phase 3 -> 4 (R_B0_S0)
//   sensor_set_kernel / sensor_get_kernel   the 126-float tables of the listed slots; a set makes the slot live
//   sensor_reset_kernel        every block to zero (phase 0)
//
// Nothing waits on another workgroup; a block is written by the threads of its own slot only (the list kernels: by the workgroups
// that list it — a slot listed twice is written twice with the same values).  A listed slot outside [0, n) is skipped.
#include "tip_sensor.h"

namespace tip {

__global__ __launch_bounds__(256) void sensor_transform_kernel(const SensorCal* __restrict__ cal, const float* __restrict__ packets,
                                                               int n_slots, float max_acc, float* __restrict__ raw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slot = i / sn::SENSORS, k = i - slot * sn::SENSORS;
    if (slot >= n_slots) return;
    const SensorCal& c = cal[slot];
    sensor_row(c.table, c.phase == sn::LIVE, packets + (size_t)slot * sn::PACKET + 7 * k, k, max_acc,
               raw + (size_t)slot * sn::RAW + 9 * k, raw + (size_t)slot * sn::RAW + 54 + 3 * k);
}

__global__ __launch_bounds__(256) void sensor_accumulate_kernel(SensorCal* __restrict__ cal, const float* __restrict__ packets,
                                                                int n_slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slot = i / sn::SENSORS, k = i - slot * sn::SENSORS;
    if (slot >= n_slots) return;
    SensorCal& c = cal[slot];
    if (c.phase != sn::HEADING && c.phase != sn::TPOSE) return;
    const float* p = packets + (size_t)slot * sn::PACKET + 7 * k;
    double S[9];
    if (!q2r<double>(p[0], p[1], p[2], p[3], S))
        for (int j = 0; j < 9; ++j) S[j] = __builtin_nan("");   // a reading without a rotation poisons the mean, as it would the demo's
    for (int j = 0; j < 9; ++j) c.sums[9 * k + j] += S[j];
    for (int j = 0; j < 3; ++j) c.sums[54 + 3 * k + j] += (double)p[4 + j];
    if (k == 0) c.count += 1;
}

__global__ __launch_bounds__(64) void sensor_begin_kernel(SensorCal* __restrict__ cal, int n_slots, const int* __restrict__ slots,
                                                          int count, int which) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n_slots) return;
    SensorCal& c = cal[slot];
    const int ph = c.phase;
    int next;
    if (which == TIP_SENSOR_HEADING && (ph == sn::UNCALIBRATED || ph == sn::HEADING_DONE || ph == sn::LIVE)) next = sn::HEADING;
    else if (which == TIP_SENSOR_TPOSE && ph == sn::HEADING_DONE) next = sn::TPOSE;
    else return;                                                 // a begin the rule does not allow: the block stays as it is
    for (int t = 0; t < sn::RAW; ++t) c.sums[t] = 0.0;
    c.count = 0;
    c.phase = next;
}

// One workgroup per list entry, one thread per sum.
__global__ __launch_bounds__(128) void sensor_finish_kernel(SensorCal* __restrict__ cal, int n_slots, const int* __restrict__ slots,
                                                            const double* __restrict__ R_Gp_B0) {
    const int slot = slots[blockIdx.x], t = threadIdx.x;
    if (slot < 0 || slot >= n_slots) return;
    SensorCal& c = cal[slot];
    __shared__ int ph_s;
    if (t == 0) ph_s = c.phase;
    __syncthreads();
    const int ph = ph_s;
    if (ph != sn::HEADING && ph != sn::TPOSE) return;
    const double cnt = (double)c.count;                          // count 0: 0 / 0, NaN tables
    if (ph == sn::HEADING) {
        if (t < sn::RAW) {
            const double m = c.sums[t] / cnt;
            c.table[t] = (float)m;                               // R_Gn_Gp = the mean matrices as they are | acc_offset
            if (t < 54) c.heading[t] = m;
        }
    } else if (t < 54) {
        const int k = t / 9, r = (t % 9) / 3, q = t % 3;
        const double* G = c.heading + 9 * k;
        const double* M = c.sums + 9 * k;
        double v = 0.0;                                          // R_B0_S0 = R_Gp_B0^T (R_Gn_Gp^T mean)
        for (int j = 0; j < 3; ++j) {
            const double gs = (G[j] * M[q] + G[3 + j] * M[3 + q] + G[6 + j] * M[6 + q]) / cnt;      // R_Gp_S0 [j][q]
            // the demo's aligned T-pose, [[0,0,1],[1,0,0],[0,1,0]] for every sensor, when no R_Gp_B0 is given
            const double b = R_Gp_B0 ? R_Gp_B0[9 * k + 3 * j + r] : (((j + 2) % 3 == r) ? 1.0 : 0.0);
            v += b * gs;
        }
        c.table[sn::T_B0_S0 + t] = (float)v;
    }
    __syncthreads();
    if (t == 0) c.phase = ph == sn::HEADING ? sn::HEADING_DONE : sn::LIVE;
}

__global__ __launch_bounds__(128) void sensor_set_kernel(SensorCal* __restrict__ cal, int n_slots, const int* __restrict__ slots,
                                                         const float* __restrict__ tables) {
    const int slot = slots[blockIdx.x], t = threadIdx.x;
    if (slot < 0 || slot >= n_slots) return;
    SensorCal& c = cal[slot];
    if (t < sn::TABLE) {
        const float v = tables[(size_t)blockIdx.x * sn::TABLE + t];
        c.table[t] = v;
        if (t < 54) c.heading[t] = (double)v;
    }
    if (t == 0) c.count = 0, c.phase = sn::LIVE;
}

__global__ __launch_bounds__(128) void sensor_get_kernel(const SensorCal* __restrict__ cal, int n_slots, const int* __restrict__ slots,
                                                         float* __restrict__ tables) {
    const int slot = slots[blockIdx.x], t = threadIdx.x;
    if (slot < 0 || slot >= n_slots || t >= sn::TABLE) return;
    tables[(size_t)blockIdx.x * sn::TABLE + t] = cal[slot].table[t];
}

__global__ __launch_bounds__(256) void sensor_reset_kernel(unsigned* __restrict__ cal, size_t words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) cal[i] = 0u;
}

}  // namespace tip

using namespace tip;

extern "C" {

static int sensor_blocks(int n_slots) { return (n_slots * sn::SENSORS + 255) / 256; }

int tip_sensor_state_bytes(int n_slots, size_t* bytes) {
    if (!bytes || tip_bad_count(n_slots)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * sizeof(SensorCal);
    return TIP_OK;
}

int tip_sensor_reset(void* cal, int n_slots, tip_stream_t stream) {
    if (!cal || tip_bad_count(n_slots) || reinterpret_cast<uintptr_t>(cal) % 8) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    const size_t words = (size_t)n_slots * sizeof(SensorCal) / 4;
    hipLaunchKernelGGL(sensor_reset_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<unsigned*>(cal), words);
    return tip_launch_status();
}

int tip_sensor_begin(void* cal, int n_slots, const int* slots, int count, int which, tip_stream_t stream) {
    if (!cal || tip_bad_count(n_slots) || count < 0 || (count > 0 && !slots) || (which != TIP_SENSOR_HEADING && which != TIP_SENSOR_TPOSE))
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_begin_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<SensorCal*>(cal), n_slots, slots, count, which);
    return tip_launch_status();
}

int tip_sensor_accumulate(void* cal, const float* packets, int n_slots, tip_stream_t stream) {
    if (!cal || !packets || tip_bad_count(n_slots)) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_accumulate_kernel, dim3(sensor_blocks(n_slots)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<SensorCal*>(cal), packets, n_slots);
    return tip_launch_status();
}

int tip_sensor_finish(void* cal, int n_slots, const int* slots, int count, const double* R_Gp_B0, tip_stream_t stream) {
    if (!cal || tip_bad_count(n_slots) || count < 0 || (count > 0 && !slots) || reinterpret_cast<uintptr_t>(R_Gp_B0) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_finish_kernel, dim3(count), dim3(128), 0, static_cast<hipStream_t>(stream), static_cast<SensorCal*>(cal),
                       n_slots, slots, R_Gp_B0);
    return tip_launch_status();
}

int tip_sensor_set(void* cal, int n_slots, const int* slots, int count, const float* tables, tip_stream_t stream) {
    if (!cal || tip_bad_count(n_slots) || count < 0 || (count > 0 && (!slots || !tables))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_set_kernel, dim3(count), dim3(128), 0, static_cast<hipStream_t>(stream), static_cast<SensorCal*>(cal),
                       n_slots, slots, tables);
    return tip_launch_status();
}

int tip_sensor_get(const void* cal, int n_slots, const int* slots, int count, float* tables_out, tip_stream_t stream) {
    if (!cal || tip_bad_count(n_slots) || count < 0 || (count > 0 && (!slots || !tables_out))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_get_kernel, dim3(count), dim3(128), 0, static_cast<hipStream_t>(stream),
                       static_cast<const SensorCal*>(cal), n_slots, slots, tables_out);
    return tip_launch_status();
}

int tip_sensor_transform(const void* cal, const float* packets, int n_slots, float max_acc, float* raw_out, tip_stream_t stream) {
    if (!cal || !packets || !raw_out || tip_bad_count(n_slots) || !(max_acc >= 0.f)) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(sensor_transform_kernel, dim3(sensor_blocks(n_slots)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const SensorCal*>(cal), packets, n_slots, max_acc, raw_out);
    return tip_launch_status();
}

}  // extern "C"
