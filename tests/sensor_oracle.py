"""fp64 oracle of the sensor front end (csrc/tip_sensor.hip; tip_amd.sensors): a numpy / scipy restatement of what the reference's live
demo computes between its socket reader and RTRunner.step (live_demo_new.py), one function per step of the demo:

    read_packet      :97-112            packet [6, 7] -> reading [72] = 6 rotation matrices (Q2R) + 6 sensor-frame accelerations
    mean_readings    :150-158           the mean of the readings of a hold
    heading          :221-226           mean -> R_Gn_Gp (the mean matrices as they are), acc_offset
    aligned_t_pose   :52-62             the known bone orientations of the aligned T-pose, R_Gp_B0
    tpose            :243-248           mean -> R_B0_S0
    transform        :161-175           reading -> the 72-column frame RTRunner.step takes

Each exists twice: per stream, sensor by sensor with one 3x3 product per line, in the order the demo does things (the functions
above), and vectorised over n streams (the *_v functions), which is what the tests run.  tests/test_sensor_cpu.py holds the two
together to 1e-15; both take their products from np.einsum, whose three-term sums round alike at any batch shape (matmul and a
written-out sum round the unclipped accelerations, up to ~40, differently in the last bit: 7e-15).

Q2R is fairmotion's (unpinned: fairmotion is no dependency of this project), which is scipy's Rotation.from_quat(q).as_matrix() with q = (x, y, z, w); A2R is
Rotation.from_rotvec(a).as_matrix().  scipy computes in fp64 whatever it is given, so the float32 evaluation the GPU test takes its
noise from (transform_v(..., dtype=np.float32)) uses q2r_formula, scipy's polynomials written out, which a CPU test pins to scipy.
"""
import numpy as np
from scipy.spatial.transform import Rotation

MAX_ACC = 10.0


def Q2R(q):
    return Rotation.from_quat(np.asarray(q, dtype=np.float64)).as_matrix()


def A2R(a):
    return Rotation.from_rotvec(np.asarray(a, dtype=np.float64)).as_matrix()


def q2r_formula(q, dtype=np.float64):
    """scipy's from_quat(q).as_matrix() written out, evaluated in `dtype` throughout: q [..., 4] (x, y, z, w) -> [..., 3, 3]."""
    q = np.asarray(q, dtype=dtype)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True, dtype=dtype))
    x, y, z, w = (q[..., i] for i in range(4))
    two = dtype(2)
    m = np.empty(q.shape[:-1] + (3, 3), dtype=dtype)
    m[..., 0, 0] = x * x - y * y - z * z + w * w
    m[..., 0, 1] = two * (x * y - z * w)
    m[..., 0, 2] = two * (x * z + y * w)
    m[..., 1, 0] = two * (x * y + z * w)
    m[..., 1, 1] = -x * x + y * y - z * z + w * w
    m[..., 1, 2] = two * (y * z - x * w)
    m[..., 2, 0] = two * (x * z - y * w)
    m[..., 2, 1] = two * (y * z + x * w)
    m[..., 2, 2] = -x * x - y * y + z * z + w * w
    return m


# ---- per stream, step by step ------------------------------------------------------------------------------------------------------
def read_packet(packet):
    """packet [42] (6 x (q0 q1 q2 q3 ax ay az)) -> reading [72]: everything in the sensors' global frame Gn."""
    q_and_a = np.asarray(packet, dtype=np.float64).reshape(6, 7)
    R = np.stack([Q2R(q_and_a[k, :4]) for k in range(6)])
    a = q_and_a[:, 4:]
    return np.concatenate((R.reshape(-1), a.reshape(-1)))


def mean_readings(readings):
    return np.asarray(readings, dtype=np.float64).mean(axis=0)


def heading(mean):
    """-> R_Gn_Gp [6,3,3] (NOT re-orthonormalised), acc_offset [6,3] (sensor frame and room frame align during this hold)."""
    return mean[:54].reshape(6, 3, 3).copy(), mean[54:].reshape(6, 3).copy()


def aligned_t_pose():
    bone = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    turn = A2R([0, 0, np.pi / 2])
    return np.stack([turn @ bone for _ in range(6)])


def tpose(mean, R_Gn_Gp, R_Gp_B0):
    R_Gn_S0 = mean[:54].reshape(6, 3, 3)
    out = np.empty((6, 3, 3))
    for k in range(6):
        R_Gp_S0 = np.einsum("ij,jk->ik", R_Gn_Gp[k].T, R_Gn_S0[k])
        out[k] = np.einsum("ij,jk->ik", R_Gp_B0[k].T, R_Gp_S0)
    return out


def transform(reading, R_Gn_Gp, acc_offset, R_B0_S0, max_acc=MAX_ACC):
    R_Gn_St = reading[:54].reshape(6, 3, 3)
    acc_St = reading[54:].reshape(6, 3)
    R_Gp_Bt, acc_Gp = np.empty((6, 3, 3)), np.empty((6, 3))
    for k in range(6):
        R_Gp_St = np.einsum("ij,jk->ik", R_Gn_Gp[k].T, R_Gn_St[k])
        R_Gp_Bt[k] = np.einsum("ij,jk->ik", R_Gp_St, R_B0_S0[k].T)
        acc_Gp[k] = np.einsum("ij,j->i", R_Gp_St, acc_St[k]) - acc_offset[k]
    acc_Gp = np.clip(acc_Gp, -max_acc, max_acc)
    return np.concatenate((R_Gp_Bt.reshape(-1), acc_Gp.reshape(-1)))


# ---- vectorised over n streams -----------------------------------------------------------------------------------------------------
def read_packet_v(packets, dtype=np.float64):
    """packets [..., 42] -> readings [..., 72]; fp64 through scipy, any other dtype through q2r_formula in that dtype."""
    p = np.asarray(packets, dtype=dtype).reshape(np.shape(packets)[:-1] + (6, 7))
    if dtype == np.float64:
        R = Q2R(p[..., :4].reshape(-1, 4)).reshape(p.shape[:-1] + (3, 3))
    else:
        R = q2r_formula(p[..., :4], dtype)
    return np.concatenate((R.reshape(p.shape[:-2] + (54,)), p[..., 4:].reshape(p.shape[:-2] + (18,))), axis=-1)


def heading_v(mean):
    return mean[..., :54].reshape(mean.shape[:-1] + (6, 3, 3)).copy(), mean[..., 54:].reshape(mean.shape[:-1] + (6, 3)).copy()


def tpose_v(mean, R_Gn_Gp, R_Gp_B0=None):
    B0 = aligned_t_pose() if R_Gp_B0 is None else np.asarray(R_Gp_B0, dtype=np.float64).reshape(6, 3, 3)
    S0 = mean[..., :54].reshape(mean.shape[:-1] + (6, 3, 3))
    R_Gp_S0 = np.einsum("...kji,...kjl->...kil", R_Gn_Gp, S0)
    return np.einsum("kji,...kjl->...kil", B0, R_Gp_S0)


def transform_v(readings, R_Gn_Gp, acc_offset, R_B0_S0, max_acc=MAX_ACC, dtype=np.float64):
    r = np.asarray(readings, dtype=dtype)
    G, off, B = (np.asarray(t, dtype=dtype) for t in (R_Gn_Gp, acc_offset, R_B0_S0))
    St = r[..., :54].reshape(r.shape[:-1] + (6, 3, 3))
    acc = r[..., 54:].reshape(r.shape[:-1] + (6, 3))
    R_Gp_St = np.einsum("...kji,...kjl->...kil", G, St)
    R_Gp_Bt = np.einsum("...kij,...klj->...kil", R_Gp_St, B)
    acc_Gp = np.clip(np.einsum("...kij,...kj->...ki", R_Gp_St, acc) - off, dtype(-max_acc), dtype(max_acc))
    return np.concatenate((R_Gp_Bt.reshape(r.shape[:-1] + (54,)), acc_Gp.reshape(r.shape[:-1] + (18,))), axis=-1)


# ---- tables: what the device keeps per slot ----------------------------------------------------------------------------------------
def pack_tables(R_Gn_Gp, acc_offset, R_B0_S0):
    """-> [..., 126] fp64: R_Gn_Gp 54 | acc_offset 18 | R_B0_S0 54 (the layout of tip_sensor_set / tip_sensor_get)."""
    lead = R_Gn_Gp.shape[:-3]
    return np.concatenate((R_Gn_Gp.reshape(lead + (54,)), acc_offset.reshape(lead + (18,)), R_B0_S0.reshape(lead + (54,))), axis=-1)


def unpack_tables(t):
    t = np.asarray(t)
    lead = t.shape[:-1]
    return t[..., :54].reshape(lead + (6, 3, 3)), t[..., 54:72].reshape(lead + (6, 3)), t[..., 72:].reshape(lead + (6, 3, 3))


def frames_from_tables(packets, tables, max_acc=MAX_ACC, dtype=np.float64):
    """The device's per-frame launch on ITS inputs: fp32 packets [n,42] and fp32 tables [n,126], evaluated in `dtype`."""
    G, off, B = unpack_tables(np.asarray(tables, dtype=np.float32))
    return transform_v(read_packet_v(np.asarray(packets, dtype=np.float32), dtype), G, off, B, max_acc, dtype)


def reorthonormalised(R):
    """The nearest rotations to the matrices R [..., 3, 3] (polar factor): what the demo does NOT do to its mean matrices."""
    U, _, Vt = np.linalg.svd(R)
    d = np.sign(np.linalg.det(U @ Vt))
    U[..., :, 2] *= d[..., None]
    return U @ Vt


# ---- inputs shared by the CPU and GPU tests ----------------------------------------------------------------------------------------
def hold_packets(rng, K, n, scatter, acc_sigma=0.5):
    """K packets [K, n, 42] of a hold: per (slot, sensor) a random base orientation, each reading `scatter` rad (normal, per axis)
    away from it; accelerations N(0, acc_sigma^2) around a per-sensor offset; quaternion lengths 0.3 .. 3."""
    base = Rotation.random(n * 6, random_state=rng)
    a0 = rng.normal(0.0, 1.0, size=(n * 6, 3))
    out = np.empty((K, n, 6, 7), dtype=np.float32)
    for t in range(K):
        q = (base * Rotation.from_rotvec(rng.normal(0.0, scatter, size=(n * 6, 3)))).as_quat()
        q = q * rng.uniform(0.3, 3.0, size=(n * 6, 1)) * rng.choice([-1.0, 1.0], size=(n * 6, 1))
        out[t, :, :, :4] = q.reshape(n, 6, 4)
        out[t, :, :, 4:] = (a0 + rng.normal(0.0, acc_sigma, size=(n * 6, 3))).reshape(n, 6, 3)
    return out.reshape(K, n, 42)


def calibrate_v(heading_packets, tpose_packets, R_Gp_B0=None):
    """The two holds in fp64 -> tables [n, 126] fp64."""
    G, off = heading_v(read_packet_v(heading_packets).mean(axis=0))
    B = tpose_v(read_packet_v(tpose_packets).mean(axis=0), G, R_Gp_B0)
    return pack_tables(G, off, B)


def frame_packets(rng, n):
    """One frame's packets [n, 42] fp32: quaternions drawn from a normal distribution and scaled to lengths 0.3 .. 3 (both signs of w
    occur), accelerations N(0, 8^2) with a few components exactly +-10."""
    q = rng.normal(size=(n, 6, 4))
    q *= rng.uniform(0.3, 3.0, size=(n, 6, 1)) / np.linalg.norm(q, axis=-1, keepdims=True)
    a = rng.normal(0.0, 8.0, size=(n, 6, 3))
    hit = rng.rand(n, 6, 3) < 0.05
    a[hit] = rng.choice([-10.0, 10.0], size=int(hit.sum()))
    return np.concatenate((q, a), axis=-1).reshape(n, 42).astype(np.float32)


def case(n, seed):
    """(packets [n,42] fp32, tables [n,126] fp32) of the transform tests: tables from the oracle's calibration of quaternions scattered
    0.02 rad around a random base (8 readings per hold), rounded to fp32 as a load() hands them to the device."""
    rng = np.random.RandomState(seed)
    tables = calibrate_v(hold_packets(rng, 8, n, 0.02), hold_packets(rng, 8, n, 0.02))
    return frame_packets(rng, n), tables.astype(np.float32)
