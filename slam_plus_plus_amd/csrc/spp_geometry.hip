// spp_geometry.hip -- everything a Gauss-Newton / Levenberg-Marquardt iteration needs besides assembly and the solve,
// so that the whole iteration stays in HBM. gfx950 only, fp64, one thread per edge / vertex / entry.
//
// Edge linearization (Jacobians column-major, r = error), each section headed by its reference and its formulas:
//   SE(2) pose-pose          CEdgePose2D           se2_linearize_kernel (vertex ids), se2_linearize_at_kernel (offsets)
//   SE(2) range-bearing      CEdgePoseLandmark2D   se2_rb_linearize_kernel
//   SE(3) pose-pose          CEdgePose3D           se3_linearize_kernel (vertex ids), se3_linearize_at_kernel (offsets)
//   SE(3) pose-landmark      CEdgePoseLandmark3D   se3_xyz_linearize_kernel
//   BA projection            CEdgeP2C3D            ba_linearize_kernel
//   BA, shared intrinsics    CEdgeP2CI3D (ternary) ba_intrinsics_linearize_kernel
//   stereo BA projection     CEdgeP2SC3D           ba_stereo_linearize_kernel
//   Sim(3) BA projection     CEdgeP2C_XYZ_Sim3_G   sim3_ba_linearize_kernel (7-wide cameras: Exp, Log and the update at the end)
// The two addressings of an edge share one __device__ body (se2_linearize_edge, se3_linearize_edge), the two mono BA
// edges share ba_p2c_edge. The kernels themselves stay named and non-templated: profiles are read by kernel name.
// Vertex updates x <- x (+) dx, each returning ||dx||^2: se2_update, se3_update, ba_update (cameras as se3_plus, points),
// ba_intrinsics_update, sim3_update (cameras as Log(Exp Exp)), slam2d_update, slam3d_update (flat states addressed by scalar offsets).
// LM scalars: edge_chi2, edge_hessian_maxdiag, lm_gain_denominator; robust (Huber) edge weights.
//
// Every scalar is a deterministic two-stage reduction: block_reduce_256 inside each workgroup (one fixed LDS tree, sum or
// max), the partials into ctx->geom_partial, one workgroup over the partials, 8 bytes to the host (fetch_scalar). The host
// wrappers at the end of each part go through one launcher (launch_per_item).
//
// The reference (functional spec, nothing is ported) has analytic Jacobians in 2D, so the device values agree with it to
// rounding; its BA and SE(3) edges use forward differences with delta = 1e-9, against which the analytic Jacobians here
// agree to the quotients' noise. tests/test_gpu_geometry_edges.py pins every kernel to a 50-digit reference instead.
// 2D helpers:
//   C2DJacobians::Absolute_to_Relative with Jacobians   include/slam/2DSolverBase.h:373-418
//   C2DJacobians::f_ClampAngle_2Pi / f_ClampAngularError_2Pi  :44-94
//   CEdgePose2D::Calculate_Jacobians_Expectation_Error  include/slam/SE2_Types.h (error = z - h(x))
//   CVertexPose2D::Operator_Plus                        include/slam/SE2_Types.h:70-74
// SE(2) pose-pose layout = what spp_assemble_device consumes: J0, J1: ne x (3 x 3) column-major, r: ne x 3;
// 2 x 24 B of gathered poses + 24 B measurement in, 168 B out; HBM-bound.

#include "spp_internal.h"
#include <math.h>

namespace spp {

__device__ __forceinline__ double clamp_angle_2pi(double a)
{
	return fmod(a, 6.283185307179586476925286766559);
}

__device__ __forceinline__ double clamp_angular_error_2pi(double e)
{
	e = clamp_angle_2pi(e);
	const double a = e - 6.283185307179586476925286766559, b = e + 6.283185307179586476925286766559;
	double m = e;
	if(fabs(a) < fabs(m)) m = a;
	if(fabs(b) < fabs(m)) m = b;
	return m;
}

// one block reduction for every kernel of this file: 256 threads, the LDS tree with offsets 128 ... 1; every thread
// returns the total, thread 0 stores it. The ORDER is fixed (thread t combines t and t + off): sums are bit-reproducible and
// tests/test_gpu_geometry_scalars.py derives its error bounds from this tree. Each kernel calls it once.
struct SumOp { __device__ __forceinline__ double operator ()(double a, double b) const { return a + b; } };
struct MaxOp { __device__ __forceinline__ double operator ()(double a, double b) const { return fmax(a, b); } };

template <class Op>
__device__ __forceinline__ double block_reduce_256(double v, Op op)
{
	__shared__ double red[256];
	red[threadIdx.x] = v;
	__syncthreads();
	for(int off = 128; off > 0; off >>= 1) {
		if((int)threadIdx.x < off)
			red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + off]);
		__syncthreads();
	}
	return red[0];
}

// the edge e between the poses at p1 and p2 (se2_linearize_kernel: poses + 3 id; se2_linearize_at_kernel: state + offset)
__device__ __forceinline__ void se2_linearize_edge(int64_t e, const double *__restrict__ p1, const double *__restrict__ p2,
	const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1, double *__restrict__ r)
{
	const double p1e = p1[0], p1n = p1[1], p1a = p1[2];
	const double de = p2[0] - p1e, dn = p2[1] - p1n;
	double s, c;
	sincos(p1a, &s, &c);
	// expectation h(x): the second pose in the frame of the first
	const double hf = c * de + s * dn, hl = -s * de + c * dn, ha = clamp_angle_2pi(p2[2] - p1a);
	const double *z = meas + 3 * e;
	r[3 * e + 0] = z[0] - hf;
	r[3 * e + 1] = z[1] - hl;
	r[3 * e + 2] = clamp_angular_error_2pi(z[2] - ha);
	// d h / d pose1 (3 x 3, column-major)
	double *a = J0 + 9 * e;
	a[0] = -c;  a[1] = s;   a[2] = 0;
	a[3] = -s;  a[4] = -c;  a[5] = 0;
	a[6] = -s * de + c * dn;
	a[7] = -c * de - s * dn;
	a[8] = -1;
	// d h / d pose2
	double *b = J1 + 9 * e;
	b[0] = c;   b[1] = -s;  b[2] = 0;
	b[3] = s;   b[4] = c;   b[5] = 0;
	b[6] = 0;   b[7] = 0;   b[8] = 1;
}

__global__ __launch_bounds__(256)
void se2_linearize_kernel(int64_t ne, const int32_t *__restrict__ v0, const int32_t *__restrict__ v1,
	const double *__restrict__ poses, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	se2_linearize_edge(e, poses + 3 * (int64_t)v0[e], poses + 3 * (int64_t)v1[e], meas, J0, J1, r);
}

// x <- x (+) dx for 2D poses (add, clamp the angle); per-workgroup partial sums of dx^2 in a FIXED order
__global__ __launch_bounds__(256)
void se2_update_kernel(int64_t nv, double *__restrict__ poses, const double *__restrict__ dx, int apply,
	double *__restrict__ partial)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	double s = 0;
	if(v < nv) {
		const double d0 = dx[3 * v], d1 = dx[3 * v + 1], d2 = dx[3 * v + 2];
		s = d0 * d0 + d1 * d1 + d2 * d2;
		if(apply) {
			poses[3 * v] += d0;
			poses[3 * v + 1] += d1;
			poses[3 * v + 2] = clamp_angle_2pi(poses[3 * v + 2] + d2);
		}
	}
	s = block_reduce_256(s, SumOp());
	if(threadIdx.x == 0 && partial)
		partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256)
void sum_partials_kernel(int64_t n, const double *__restrict__ partial, double *__restrict__ out)
{
	double s = 0;
	for(int64_t i = threadIdx.x; i < n; i += 256) // fixed assignment, fixed order: bit-reproducible
		s += partial[i];
	s = block_reduce_256(s, SumOp());
	if(threadIdx.x == 0)
		out[0] = s;
}

// --------------------------------------------------------------------------------------------------
// Bundle adjustment: projection edge CEdgeP2C3D (camera 6D pose [t | axis-angle], world -> camera,
// + 5 constant intrinsics fx fy cx cy k; point XYZ). Reference (functional spec):
//   CBAJacobians::Project_P2C               include/slam/BASolverBase.h:260-325 (model), :559-620 (Jacobians)
//     x = R(aa) X + t ; d = (fx x/z, fy y/z) ; k' = k / ((fx + fy) / 2) ; uv = c + (1 + |d|^2 k') d
//   its Jacobians are FORWARD DIFFERENCES (delta = 1e-9) over the camera increment
//     cam (+) delta = C3DJacobians::Relative_to_Absolute(cam, delta): t' = t + R dt, R' = R exp(dr)
//     (include/slam/3DSolverBase.h:807-850) and over an additive point increment.
// Here the same derivatives are ANALYTIC:  d uv / d x = ((1 + r2 k') I + 2 k' d d^T) [fx/z 0 -fx x/z^2; 0 fy/z -fy y/z^2]
//   J_cam = d uv/d x [ R | -R [X]x ],  J_pt = d uv/d x R,   r = z - uv.
// They agree with the reference's difference quotients to the quotients' own noise (~1e-7 relative:
// tests/test_gpu_ba_geometry.py compares with golden vectors produced by the reference).
// One thread per observation: 11 + 3 gathered doubles + 16 B in, 160 B out (J0 2x6, J1 2x3 column-major, r).
// --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void axis_angle_to_rot(const double *a, double *R) // row-major 3 x 3
{
	const double x = a[0], y = a[1], z = a[2], th2 = x * x + y * y + z * z, th = sqrt(th2);
	double A, B; // sin(th)/th, (1 - cos(th))/th^2
	if(th < 1e-6) {
		A = 1.0 - th2 * (1.0 / 6.0);
		B = 0.5 - th2 * (1.0 / 24.0);
	} else {
		double s, c;
		sincos(th, &s, &c);
		A = s / th;
		const double sh = sin(0.5 * th);
		B = 2.0 * sh * sh / th2;
	}
	R[0] = 1 - B * (y * y + z * z); R[1] = B * x * y - A * z;       R[2] = B * x * z + A * y;
	R[3] = B * x * y + A * z;       R[4] = 1 - B * (x * x + z * z); R[5] = B * y * z - A * x;
	R[6] = B * x * z - A * y;       R[7] = B * y * z + A * x;       R[8] = 1 - B * (x * x + y * y);
}

// one observation of Project_P2C: a = J0 (2x6), b = J1 (2x3), both column-major, r = z - uv; xyz (may be dead) <- the point in
// the camera frame as (x, y, 1 / z). ONE body for spp_ba_linearize_device and spp_ba_intrinsics_linearize_device.
__device__ __forceinline__ void ba_p2c_edge(const double *__restrict__ cam, const double *__restrict__ in,
	const double *__restrict__ X, const double *__restrict__ meas, double *__restrict__ a, double *__restrict__ b,
	double *__restrict__ r, double *xyz)
{
	double R[9];
	axis_angle_to_rot(cam + 3, R);
	const double X0 = X[0], X1 = X[1], X2 = X[2];
	const double x = R[0] * X0 + R[1] * X1 + R[2] * X2 + cam[0];
	const double y = R[3] * X0 + R[4] * X1 + R[5] * X2 + cam[1];
	const double z = R[6] * X0 + R[7] * X1 + R[8] * X2 + cam[2];
	const double fx = in[0], fy = in[1], k = in[4] / (0.5 * (fx + fy));
	const double iz = 1.0 / z, d0 = fx * x * iz, d1 = fy * y * iz, r2 = d0 * d0 + d1 * d1, g = 1.0 + r2 * k;
	r[0] = meas[0] - (in[2] + g * d0);
	r[1] = meas[1] - (in[3] + g * d1);
	// d uv / d x (2 x 3): D * Jd
	const double D00 = g + 2 * k * d0 * d0, D01 = 2 * k * d0 * d1, D11 = g + 2 * k * d1 * d1;
	const double a0 = fx * iz, a2 = -fx * x * iz * iz, b1 = fy * iz, b2 = -fy * y * iz * iz; // Jd = [a0 0 a2; 0 b1 b2]
	const double P[6] = {D00 * a0, D01 * b1, D00 * a2 + D01 * b2,   // row 0
	                     D01 * a0, D11 * b1, D01 * a2 + D11 * b2};  // row 1
	// PR = P R (2 x 3) = d uv / d dt = d uv / d X
	double PR[6];
#pragma unroll
	for(int i = 0; i < 2; ++ i)
#pragma unroll
		for(int j = 0; j < 3; ++ j)
			PR[3 * i + j] = P[3 * i] * R[j] + P[3 * i + 1] * R[3 + j] + P[3 * i + 2] * R[6 + j];
#pragma unroll
	for(int j = 0; j < 3; ++ j) {
		a[2 * j] = PR[j];
		a[2 * j + 1] = PR[3 + j];
		b[2 * j] = PR[j];
		b[2 * j + 1] = PR[3 + j];
	}
	// d uv / d dr = -PR [X]x : columns (PR x X) component-wise: -PR * [X]x = [PR_1 X2 - PR_2 X1, PR_2 X0 - PR_0 X2, PR_0 X1 - PR_1 X0] * (-1) ...
#pragma unroll
	for(int i = 0; i < 2; ++ i) {
		const double p0 = PR[3 * i], p1 = PR[3 * i + 1], p2 = PR[3 * i + 2];
		// -(p^T [X]x) with [X]x = [0 -X2 X1; X2 0 -X0; -X1 X0 0]: p^T [X]x = (p1 X2 - p2 X1, p2 X0 - p0 X2, p0 X1 - p1 X0)
		a[6 + i] = -(p1 * X2 - p2 * X1);
		a[8 + i] = -(p2 * X0 - p0 * X2);
		a[10 + i] = -(p0 * X1 - p1 * X0);
	}
	xyz[0] = x; xyz[1] = y; xyz[2] = iz;
}

__global__ __launch_bounds__(256)
void ba_linearize_kernel(int64_t no, const int32_t *__restrict__ cam_of, const int32_t *__restrict__ pt_of,
	const double *__restrict__ cams, const double *__restrict__ intr, const double *__restrict__ pts,
	const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= no)
		return;
	double xyz[3];
	ba_p2c_edge(cams + 6 * (int64_t)cam_of[e], intr + 5 * (int64_t)cam_of[e], pts + 3 * (int64_t)pt_of[e], meas + 2 * e,
		J0 + 12 * e, J1 + 6 * e, r + 2 * e, xyz);
}

// --------------------------------------------------------------------------------------------------
// Self-calibrating bundle adjustment: the ternary edge CEdgeP2CI3D (include/slam/BA_Types.h:562-700) between a camera
// CVertexCam (6), a point CVertexXYZ (3) and an intrinsics vertex CVertexIntrinsics (5: fx fy cx cy kappa, :141-206) that
// several cameras may share. Projection, r, J0 and J1 are those of Project_P2C above -- the same device function, with the
// intrinsics taken from the edge's third vertex. J2 = d uv / d (fx fy cx cy kappa) w.r.t. the plain increment of
// Relative_to_Absolute_Intrinsics (BASolverBase.h:204-212), analytic where the reference takes forward differences with
// delta = 1e-9 (:690-759). With p = (x/z, y/z), d = (fx p0, fy p1), F = fx + fy, k = kappa / (0.5 F), r2 = |d|^2, g = 1 + r2 k:
//   d uv / d fx = g (p0, 0) + d (2 k d0 p0 - r2 k / F)      d uv / d cx = (1, 0)
//   d uv / d fy = g (0, p1) + d (2 k d1 p1 - r2 k / F)      d uv / d cy = (0, 1)      d uv / d kappa = d r2 / (0.5 F)
// Nothing is divided by r: a point on the optical axis gives finite (zero) columns. Inside the library the vertex is 6 wide:
// J2 is 2x6 column-major and its last column, the inert coordinate, is written as zeros.
// J2 reads x, y, 1/z through an empty asm statement: its arithmetic then shares no subexpression with the body above,
// which is therefore contracted into the same FMAs in both kernels (J0, J1, r bit-identical between them).
// --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double opaque_copy(double x)
{
	asm volatile("" : "+v"(x));
	return x;
}

__global__ __launch_bounds__(256)
void ba_intrinsics_linearize_kernel(int64_t no, const int32_t *__restrict__ cam_of, const int32_t *__restrict__ pt_of,
	const int32_t *__restrict__ intr_of, const double *__restrict__ cams, const double *__restrict__ intr,
	const double *__restrict__ pts, const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1,
	double *__restrict__ J2, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= no)
		return;
	const double *in = intr + 5 * (int64_t)intr_of[e];
	double xyz[3];
	ba_p2c_edge(cams + 6 * (int64_t)cam_of[e], in, pts + 3 * (int64_t)pt_of[e], meas + 2 * e, J0 + 12 * e, J1 + 6 * e, r + 2 * e, xyz);
	const double x = opaque_copy(xyz[0]), y = opaque_copy(xyz[1]), iz = opaque_copy(xyz[2]);
	const double fx = opaque_copy(in[0]), fy = opaque_copy(in[1]), kappa = opaque_copy(in[4]);
	const double p0 = x * iz, p1 = y * iz, d0 = fx * p0, d1 = fy * p1, F = fx + fy, k = kappa / (0.5 * F);
	const double r2 = d0 * d0 + d1 * d1, g = 1.0 + r2 * k, kF = r2 * k / F;
	const double sx = 2.0 * k * d0 * p0 - kF, sy = 2.0 * k * d1 * p1 - kF, sk = r2 / (0.5 * F);
	double *c = J2 + 12 * e;
	c[0] = g * p0 + d0 * sx; c[1] = d1 * sx;          // fx
	c[2] = d0 * sy;          c[3] = g * p1 + d1 * sy; // fy
	c[4] = 1.0; c[5] = 0.0;                           // cx
	c[6] = 0.0; c[7] = 1.0;                           // cy
	c[8] = d0 * sk; c[9] = d1 * sk;                   // kappa
	c[10] = 0.0; c[11] = 0.0;                         // inert
}

// CVertexIntrinsics::Operator_Plus AS WRITTEN (BA_Types.h:170-185): fx fy cx cy are plain sums; kappa is divided by
// 0.5 fx fy -- the PRODUCT, not the 0.5 (fx + fy) of the projection -- of the old state, incremented by its delta divided
// alike, and multiplied by 0.5 fx fy of the new state. One thread per intrinsics vertex; dx at dxoff[i] .. + 5.
__global__ __launch_bounds__(256)
void ba_update_intrinsics_kernel(int64_t ni, double *__restrict__ intr, const int64_t *__restrict__ dxoff, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= ni)
		return;
	double *v = intr + 5 * i;
	const double *d = dx + dxoff[i];
	const double den = 0.5 * (v[0] * v[1]);
	const double dn = v[4] / den + d[4] / den;
	const double fx = v[0] + d[0], fy = v[1] + d[1];
	v[0] = fx;
	v[1] = fy;
	v[2] += d[2];
	v[3] += d[3];
	v[4] = dn * (0.5 * (fx * fy));
}

// ||dx||^2 over the 5 live coordinates of every intrinsics vertex: one workgroup, fixed assignment, fixed tree
__global__ __launch_bounds__(256)
void intrinsics_norm2_kernel(int64_t ni, const int64_t *__restrict__ dxoff, const double *__restrict__ dx, double *__restrict__ out)
{
	double s = 0;
	for(int64_t q = threadIdx.x; q < 5 * ni; q += 256) {
		const double v = dx[dxoff[q / 5] + q % 5];
		s += v * v;
	}
	s = block_reduce_256(s, SumOp());
	if(threadIdx.x == 0)
		out[0] = s;
}

// --------------------------------------------------------------------------------------------------
// Stereo bundle adjustment: projection edge CEdgeP2SC3D (include/slam/BA_Types.h:705-811) between a stereo camera
// CVertexSCam (6D pose [t | axis-angle], world -> LEFT camera, + 6 constant intrinsics fx fy cx cy d b, b the baseline)
// and a point XYZ. Reference (functional spec):
//   CBAJacobians::Project_P2SC               include/slam/BASolverBase.h:462-537 (model), :781-841 (Jacobians)
//     x = R X + t ; q = p - c = (fx x0 / x2, fy x1 / x2) ; k = d / ((fx + fy) / 2) ; rho = |q| ; uv = c + (1 + rho k) q
//     (the distortion is LINEAR in rho here, where Project_P2C has rho^2); the right camera sees the point moved by
//     -b (row 0 of R)^T through the same projection and distortion with its own rho; expectation (uv0, uv1, uv_right0).
//   Since R (row 0 of R)^T = e0, the moved point in the camera frame is x - b e0: THAT form is evaluated here (one
//   rotation instead of two), and it holds for the incremented camera too (R' R'^T e0 = e0), so the right camera
//   shares d x / d increment with the left one.
//   The reference's Jacobians are FORWARD DIFFERENCES (delta = 1e-9) over cam (+) delta = Relative_to_Absolute
//   (t' = t + R dt, R' = R exp(dr), 3DSolverBase.h:807-850) and over an additive point increment. Here ANALYTIC:
//     d uv / d q = (1 + rho k) I + k q n^T,  n = q / rho  and  n = 0 at rho = 0, where the term vanishes (|q n^T| = rho):
//     a point on the optical axis gives finite Jacobians; d q / d x = [fx/x2 0 -fx x0/x2^2; 0 fy/x2 -fy x1/x2^2];
//     P (3 x 3) = rows 0, 1 of the left chain and row 0 of the right one (at x - b e0);
//     J_cam = P [ R | -R [X]x ],  J_pt = P R,  r = z - e.
// One thread per observation: 12 + 3 gathered doubles + 24 B in, 240 B out (J0 3x6, J1 3x3 column-major, r 3):
// the (6,3,3) group of spp_assemble_device.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void ba_stereo_linearize_kernel(int64_t no, const int32_t *__restrict__ cam_of, const int32_t *__restrict__ pt_of,
	const double *__restrict__ cams, const double *__restrict__ intr, const double *__restrict__ pts,
	const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= no)
		return;
	const double *cam = cams + 6 * (int64_t)cam_of[e], *in = intr + 6 * (int64_t)cam_of[e], *X = pts + 3 * (int64_t)pt_of[e];
	double R[9];
	axis_angle_to_rot(cam + 3, R);
	const double X0 = X[0], X1 = X[1], X2 = X[2];
	const double x = R[0] * X0 + R[1] * X1 + R[2] * X2 + cam[0];
	const double y = R[3] * X0 + R[4] * X1 + R[5] * X2 + cam[1];
	const double z = R[6] * X0 + R[7] * X1 + R[8] * X2 + cam[2];
	const double fx = in[0], fy = in[1], k = in[4] / (0.5 * (fx + fy)), xr = x - in[5];
	const double iz = 1.0 / z, q0 = fx * x * iz, q1 = fy * y * iz, s0 = fx * xr * iz; // left q, right (s0, q1)
	const double rho = sqrt(q0 * q0 + q1 * q1), rhor = sqrt(s0 * s0 + q1 * q1), g = 1.0 + rho * k, gr = 1.0 + rhor * k;
	r[3 * e] = meas[3 * e] - (in[2] + g * q0);
	r[3 * e + 1] = meas[3 * e + 1] - (in[3] + g * q1);
	r[3 * e + 2] = meas[3 * e + 2] - (in[2] + gr * s0);
	// unit vectors q / rho, 0 at rho = 0 (|q_i| <= rho: the quotient cannot overflow)
	const double n0 = (rho > 0) ? q0 / rho : 0.0, n1 = (rho > 0) ? q1 / rho : 0.0;
	const double m0 = (rhor > 0) ? s0 / rhor : 0.0, m1 = (rhor > 0) ? q1 / rhor : 0.0;
	const double D00 = g + k * q0 * n0, D01 = k * q0 * n1, D11 = g + k * q1 * n1; // symmetric: q0 n1 = q1 n0
	const double E0 = gr + k * s0 * m0, E1 = k * s0 * m1;                        // row 0 of the right camera's
	const double a0 = fx * iz, a2 = -fx * x * iz * iz, b1 = fy * iz, b2 = -fy * y * iz * iz, c2 = -fx * xr * iz * iz;
	const double P[9] = {D00 * a0, D01 * b1, D00 * a2 + D01 * b2,
	                     D01 * a0, D11 * b1, D01 * a2 + D11 * b2,
	                     E0 * a0,  E1 * b1,  E0 * c2 + E1 * b2};
	double PR[9]; // P R = d e / d dt = d e / d X
#pragma unroll
	for(int i = 0; i < 3; ++ i)
#pragma unroll
		for(int j = 0; j < 3; ++ j)
			PR[3 * i + j] = P[3 * i] * R[j] + P[3 * i + 1] * R[3 + j] + P[3 * i + 2] * R[6 + j];
	double *a = J0 + 18 * e, *b = J1 + 9 * e;
#pragma unroll
	for(int j = 0; j < 3; ++ j)
#pragma unroll
		for(int i = 0; i < 3; ++ i) {
			a[3 * j + i] = PR[3 * i + j];
			b[3 * j + i] = PR[3 * i + j];
		}
	// d e / d dr = -PR [X]x, row by row as in ba_linearize_kernel
#pragma unroll
	for(int i = 0; i < 3; ++ i) {
		const double p0 = PR[3 * i], p1 = PR[3 * i + 1], p2 = PR[3 * i + 2];
		a[9 + i] = -(p1 * X2 - p2 * X1);
		a[12 + i] = -(p2 * X0 - p0 * X2);
		a[15 + i] = -(p0 * X1 - p1 * X0);
	}
}

// camera and 6D pose (+): t' = t + R dt, R' = R exp(dr) through unit quaternions with w >= 0 (the reference's
// AxisAngle_to_Quat / Quat_to_AxisAngle, 3DSolverBase.h:477-502,557+); se3_plus serves se3_update_kernel and slam3d_pose_plus_kernel
__device__ __forceinline__ void aa_to_quat(const double *a, double *q) // q = (w, x, y, z)
{
	const double th = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	double c, s_over;
	if(th < 1e-12) {
		c = 1.0;
		s_over = 0.5;
	} else {
		double sh;
		sincos(0.5 * th, &sh, &c);
		s_over = sh / th;
		if(c < 0) {
			c = -c;
			s_over = -s_over;
		}
	}
	q[0] = c; q[1] = a[0] * s_over; q[2] = a[1] * s_over; q[3] = a[2] * s_over;
}

__device__ __forceinline__ void quat_to_aa(double w, double vx, double vy, double vz, double *a)
{
	if(w < 0) {
		w = -w; vx = -vx; vy = -vy; vz = -vz;
	}
	const double vn = sqrt(vx * vx + vy * vy + vz * vz);
	const double scale = (vn < 1e-12) ? 2.0 : 2.0 * atan2(vn, w) / vn;
	a[0] = vx * scale; a[1] = vy * scale; a[2] = vz * scale;
}

__device__ __forceinline__ void quat_mul(const double *p, const double *q, double *o) // o = p q, (w, x, y, z)
{
	o[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
	o[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
	o[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
	o[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

// 6D pose (+): t' = t + R dt, R' = R exp(dr) (CVertexPose3D::Operator_Plus, SE3_Types.h:44-47); o may be p
__device__ __forceinline__ void se3_plus(const double *p, const double *d, double *o)
{
	double R[9], q1[4], q2[4], q[4];
	axis_angle_to_rot(p + 3, R);
	const double t0 = p[0] + (R[0] * d[0] + R[1] * d[1] + R[2] * d[2]);
	const double t1 = p[1] + (R[3] * d[0] + R[4] * d[1] + R[5] * d[2]);
	const double t2 = p[2] + (R[6] * d[0] + R[7] * d[1] + R[8] * d[2]);
	aa_to_quat(p + 3, q1);
	aa_to_quat(d + 3, q2);
	quat_mul(q1, q2, q);
	o[0] = t0; o[1] = t1; o[2] = t2;
	quat_to_aa(q[0], q[1], q[2], q[3], o + 3);
}

__global__ __launch_bounds__(256)
void ba_update_cams_kernel(int64_t nc, double *__restrict__ cams, const int64_t *__restrict__ dxoff, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= nc)
		return;
	// se3_plus written out, apart from the quaternion product: the compiler contracts vx^2 + vy^2 + vz^2 into other FMAs
	// behind se3_plus / quat_to_aa than it does here, and a camera would move by an ulp against earlier builds
	double *cam = cams + 6 * i;
	const double *d = dx + dxoff[i];
	double R[9], q1[4], q2[4], q[4];
	axis_angle_to_rot(cam + 3, R);
	cam[0] += R[0] * d[0] + R[1] * d[1] + R[2] * d[2];
	cam[1] += R[3] * d[0] + R[4] * d[1] + R[5] * d[2];
	cam[2] += R[6] * d[0] + R[7] * d[1] + R[8] * d[2];
	aa_to_quat(cam + 3, q1);
	aa_to_quat(d + 3, q2);
	quat_mul(q1, q2, q);
	double w = q[0], vx = q[1], vy = q[2], vz = q[3];
	if(w < 0) {
		w = -w; vx = -vx; vy = -vy; vz = -vz;
	}
	const double vn = sqrt(vx * vx + vy * vy + vz * vz);
	const double scale = (vn < 1e-12) ? 2.0 : 2.0 * atan2(vn, w) / vn;
	cam[3] = vx * scale;
	cam[4] = vy * scale;
	cam[5] = vz * scale;
}

__global__ __launch_bounds__(256)
void ba_update_points_kernel(int64_t np, double *__restrict__ pts, const int64_t *__restrict__ dxoff, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= np)
		return;
	const double *d = dx + dxoff[i];
	pts[3 * i] += d[0];
	pts[3 * i + 1] += d[1];
	pts[3 * i + 2] += d[2];
}

__global__ __launch_bounds__(256)
void norm2_partial_kernel(int64_t n, const double *__restrict__ v, double *__restrict__ partial)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const double s = block_reduce_256((i < n) ? v[i] * v[i] : 0.0, SumOp());
	if(threadIdx.x == 0)
		partial[blockIdx.x] = s;
}

// --------------------------------------------------------------------------------------------------
// SE(3) pose-pose edge CEdgePose3D (vertices [t | axis-angle]). Reference (functional spec):
//   expectation e = C3DJacobians::Absolute_to_Relative(v1, v2): e_t = R1^T (t2 - t1), e_r = log(R1^T R2)
//   Jacobians: forward differences (delta = 1e-9) over v (+) d = Relative_to_Absolute(v, d)
//                                                     include/slam/3DSolverBase.h:1331-1371, :807-850
//   error: [z_t - e_t ; log(R(z_r) R(e_r)^T)]         include/slam/SE3_Types.h:264-286
// Here analytic (R_e = R1^T R2, Jr^-1 = inverse right Jacobian of SO(3) at e_r):
//   d e / d d1 = [ -I   [e_t]x ; 0  -Jr^-1 R_e^T ],   d e / d d2 = [ R_e  0 ; 0  Jr^-1 ]
// agreeing with the reference's difference quotients to their noise (tests/test_gpu_se3_geometry.py).
// One thread per edge; J0, J1: 6 x 6 column-major, r: 6.
// --------------------------------------------------------------------------------------------------
// the edge e between the poses at p1 and p2 (se3_linearize_kernel: poses + 6 id; se3_linearize_at_kernel: state + offset)
__device__ __forceinline__ void se3_linearize_edge(int64_t e, const double *__restrict__ p1, const double *__restrict__ p2,
	const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1, double *__restrict__ r)
{
	const double *z = meas + 6 * e;
	double R1[9], R2[9], Re[9];
	axis_angle_to_rot(p1 + 3, R1);
	axis_angle_to_rot(p2 + 3, R2);
	const double d0 = p2[0] - p1[0], d1 = p2[1] - p1[1], d2 = p2[2] - p1[2];
	const double et[3] = {R1[0] * d0 + R1[3] * d1 + R1[6] * d2, R1[1] * d0 + R1[4] * d1 + R1[7] * d2,
		R1[2] * d0 + R1[5] * d1 + R1[8] * d2}; // R1^T (t2 - t1)
#pragma unroll
	for(int i = 0; i < 3; ++ i)
#pragma unroll
		for(int j = 0; j < 3; ++ j)
			Re[3 * i + j] = R1[i] * R2[j] + R1[3 + i] * R2[3 + j] + R1[6 + i] * R2[6 + j]; // R1^T R2
	double q1[4], q2[4], qe[4], er[3];
	aa_to_quat(p1 + 3, q1);
	aa_to_quat(p2 + 3, q2);
	q1[1] = -q1[1]; q1[2] = -q1[2]; q1[3] = -q1[3]; // conjugate
	quat_mul(q1, q2, qe);
	quat_to_aa(qe[0], qe[1], qe[2], qe[3], er);
	// error
	double qz[4], qec[4] = {qe[0], -qe[1], -qe[2], -qe[3]}, qr[4], rr[3];
	if(qec[0] < 0) { // the canonical (w >= 0) representative of the expectation, as quat_to_aa / aa_to_quat round-trip
		qec[0] = -qec[0]; qec[1] = -qec[1]; qec[2] = -qec[2]; qec[3] = -qec[3];
	}
	aa_to_quat(z + 3, qz);
	quat_mul(qz, qec, qr);
	quat_to_aa(qr[0], qr[1], qr[2], qr[3], rr);
	double *ro = r + 6 * e;
	ro[0] = z[0] - et[0]; ro[1] = z[1] - et[1]; ro[2] = z[2] - et[2];
	ro[3] = rr[0]; ro[4] = rr[1]; ro[5] = rr[2];
	// Jr^-1(e_r) = I + 1/2 K + c K^2, K = [e_r]x, c = 1/th^2 - (1 + cos th) / (2 th sin th)
	const double th2 = er[0] * er[0] + er[1] * er[1] + er[2] * er[2], th = sqrt(th2);
	double c;
	if(th < 1e-4)
		c = 1.0 / 12.0 + th2 * (1.0 / 720.0);
	else {
		double sn, cs;
		sincos(th, &sn, &cs);
		c = 1.0 / th2 - (1.0 + cs) / (2.0 * th * sn);
	}
	const double x = er[0], y = er[1], zz = er[2];
	double Ji[9] = { // I + K/2 + c K^2 (row-major)
		1 - c * (y * y + zz * zz), -0.5 * zz + c * x * y,      0.5 * y + c * x * zz,
		0.5 * zz + c * x * y,      1 - c * (x * x + zz * zz),  -0.5 * x + c * y * zz,
		-0.5 * y + c * x * zz,     0.5 * x + c * y * zz,       1 - c * (x * x + y * y)};
	double *a = J0 + 36 * e, *b = J1 + 36 * e;
#pragma unroll
	for(int q = 0; q < 36; ++ q) {
		a[q] = 0;
		b[q] = 0;
	}
	// J0 = [ -I  [e_t]x ; 0  -Ji Re^T ]   (column-major: element (row, col) at row + 6 col)
	a[0 + 6 * 0] = -1; a[1 + 6 * 1] = -1; a[2 + 6 * 2] = -1;
	a[0 + 6 * 4] = -et[2]; a[0 + 6 * 5] = et[1];
	a[1 + 6 * 3] = et[2];  a[1 + 6 * 5] = -et[0];
	a[2 + 6 * 3] = -et[1]; a[2 + 6 * 4] = et[0];
#pragma unroll
	for(int i = 0; i < 3; ++ i)
#pragma unroll
		for(int j = 0; j < 3; ++ j) {
			a[(3 + i) + 6 * (3 + j)] = -(Ji[3 * i] * Re[3 * j] + Ji[3 * i + 1] * Re[3 * j + 1] + Ji[3 * i + 2] * Re[3 * j + 2]);
			b[i + 6 * j] = Re[3 * i + j];
			b[(3 + i) + 6 * (3 + j)] = Ji[3 * i + j];
		}
}

__global__ __launch_bounds__(256)
void se3_linearize_kernel(int64_t ne, const int32_t *__restrict__ v0, const int32_t *__restrict__ v1,
	const double *__restrict__ poses, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	se3_linearize_edge(e, poses + 6 * (int64_t)v0[e], poses + 6 * (int64_t)v1[e], meas, J0, J1, r);
}

__global__ __launch_bounds__(256)
void se3_update_kernel(int64_t nv, double *__restrict__ poses, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= nv)
		return;
	se3_plus(poses + 6 * i, dx + 6 * i, poses + 6 * i);
}

// --------------------------------------------------------------------------------------------------
// Scalars the Levenberg-Marquardt control needs (reference include/slam/NonlinearSolver_Lambda_LM.h):
//   chi2 = sum_e r_e^T Omega_e r_e                                  (f_Error, :1078-1095)
//   alpha0 input = max_e max diag(J_i^T Omega J_i)                  (f_InitialDamping, :151-199)
//   gain denominator = dx . (alpha dx + eta)                        (Aftermath, :204-222)
// Deterministic two-stage reductions (per-workgroup partials in a fixed order, then one workgroup).
// --------------------------------------------------------------------------------------------------
template <int RD>
__global__ __launch_bounds__(256)
void edge_chi2_kernel(int64_t ne, const double *__restrict__ r, const double *__restrict__ Om, double *__restrict__ partial)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	double s = 0;
	if(e < ne) {
		const double *re = r + RD * e, *oe = Om + RD * RD * e;
#pragma unroll
		for(int i = 0; i < RD; ++ i) {
			double t = 0;
#pragma unroll
			for(int j = 0; j < RD; ++ j)
				t += oe[i + RD * j] * re[j];
			s += re[i] * t;
		}
	}
	s = block_reduce_256(s, SumOp());
	if(threadIdx.x == 0)
		partial[blockIdx.x] = s;
}

template <int RD, int D>
__device__ __forceinline__ double max_hdiag(const double *J, const double *Om)
{
	double m = 0;
#pragma unroll
	for(int c = 0; c < D; ++ c) { // (J^T Omega J)_cc, J: RD x D column-major
		double s = 0;
#pragma unroll
		for(int i = 0; i < RD; ++ i) {
			double t = 0;
#pragma unroll
			for(int j = 0; j < RD; ++ j)
				t += Om[i + RD * j] * J[j + RD * c];
			s += J[i + RD * c] * t;
		}
		m = fmax(m, s);
	}
	return m;
}

template <int RD, int D0, int D1>
__global__ __launch_bounds__(256)
void edge_maxdiag_kernel(int64_t ne, const double *__restrict__ J0, const double *__restrict__ J1,
	const double *__restrict__ Om, double *__restrict__ partial)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	double m = 0;
	if(e < ne)
		m = fmax(max_hdiag<RD, D0>(J0 + RD * D0 * e, Om + RD * RD * e), max_hdiag<RD, D1>(J1 + RD * D1 * e, Om + RD * RD * e));
	m = block_reduce_256(m, MaxOp());
	if(threadIdx.x == 0)
		partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(256)
void max_partials_kernel(int64_t n, const double *__restrict__ partial, double *__restrict__ out)
{
	double m = 0;
	for(int64_t i = threadIdx.x; i < n; i += 256)
		m = fmax(m, partial[i]);
	m = block_reduce_256(m, MaxOp());
	if(threadIdx.x == 0)
		out[0] = m;
}

__global__ __launch_bounds__(256)
void gain_partial_kernel(int64_t n, const double *__restrict__ dx, const double *__restrict__ rhs, double alpha,
	double *__restrict__ partial)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const double s = block_reduce_256((i < n) ? dx[i] * (alpha * dx[i] + rhs[i]) : 0.0, SumOp());
	if(threadIdx.x == 0)
		partial[blockIdx.x] = s;
}

// --------------------------------------------------------------------------------------------------
// Host side. ONE launcher, ONE second stage, ONE read-back:
//   launch_per_item   kernel(n, ...) over ceil(n / 256) workgroups of 256 on ctx->stream; nothing for n = 0
//   geom_partial      p[0] = the scalar, p[1 .. nwg] = the first stage's partials, anything else behind them
//   reduce_partials   sum_partials_kernel / max_partials_kernel over the partials into p[0] (enqueued)
//   enqueue_norm2     ||v||^2 of a flat vector into p[0] (enqueued), `extra` doubles kept behind the partials
//   fetch_scalar      p[0] to the host: the one stream synchronisation of an entry point that returns a scalar
// --------------------------------------------------------------------------------------------------
static inline int64_t n_workgroups(int64_t n)
{
	return (n + 255) / 256;
}

template <class Kernel, class... Args>
static void launch_over(spp_ctx *ctx, Kernel kernel, int64_t n_threads, Args... args)
{
	if(!n_threads)
		return;
	hipLaunchKernelGGL(kernel, dim3((unsigned)n_workgroups(n_threads)), dim3(256), 0, ctx->stream, args...);
	SPP_HIP_CHECK(hipGetLastError());
}

template <class Kernel, class... Args>
static void launch_per_item(spp_ctx *ctx, Kernel kernel, int64_t n, Args... args)
{
	launch_over(ctx, kernel, n, n, args...);
}

static double *reserve_partials(spp_ctx *ctx, int64_t n, size_t extra = 0)
{
	ctx->geom_partial.reserve((size_t)n_workgroups(n) + 1 + extra);
	return ctx->geom_partial.p + 1;
}

static void reduce_partials(spp_ctx *ctx, int64_t n, bool take_max = false)
{
	hipLaunchKernelGGL(take_max ? max_partials_kernel : sum_partials_kernel, dim3(1), dim3(256), 0, ctx->stream, n_workgroups(n),
		ctx->geom_partial.p + 1, ctx->geom_partial.p);
}

static void enqueue_norm2(spp_ctx *ctx, int64_t n, const double *d_v, size_t extra = 0)
{
	double *part = reserve_partials(ctx, n, extra);
	if(!n)
		return;
	launch_per_item(ctx, norm2_partial_kernel, n, d_v, part);
	reduce_partials(ctx, n);
}

static double fetch_scalar(spp_ctx *ctx)
{
	double h = 0;
	SPP_HIP_CHECK(hipGetLastError());
	SPP_HIP_CHECK(hipMemcpyAsync(&h, ctx->geom_partial.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	SPP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return h;
}

// ---- robust kernels on the error norm (include/geometry/RobustLoss.h; mix-in include/slam/RobustUtils.h:368-400):
// w_e = kernel(||r_e|| / scale). kind 0: Huber, w = 1 for x <= k, k / x beyond (CHuberLoss::operator (), :100-104)
__global__ __launch_bounds__(256)
void edge_robust_weight_kernel(int64_t ne, int rd, int kind, double scale, double param, const double *__restrict__ r,
	double *__restrict__ w)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	double s = 0;
	for(int i = 0; i < rd; ++ i)
		s += r[e * rd + i] * r[e * rd + i]; // Eigen's norm(): sqrt of the sum of squares, in order
	const double x = sqrt(s) / scale;
	w[e] = (x <= param) ? 1.0 : param / x;
	(void)kind;
}

void edge_robust_weights(spp_ctx *ctx, int64_t ne, int rd, int kind, double scale, double param, const double *d_r, double *d_w)
{
	SPP_REQUIRE(kind == 0, SPP_E_UNSUPPORTED, "robust weights: only the Huber kernel (kind 0) is instantiated");
	SPP_REQUIRE(scale > 0 && param > 0 && rd > 0, SPP_E_BADARG, "robust weights: scale, parameter and residual dimension must be positive");
	launch_per_item(ctx, edge_robust_weight_kernel, ne, rd, kind, scale, param, d_r, d_w);
}

double edge_chi2(spp_ctx *ctx, int64_t ne, int rd, const double *d_r, const double *d_Om)
{
	if(!ne)
		return 0;
	double *part = reserve_partials(ctx, ne);
	if(rd == 1) launch_per_item(ctx, edge_chi2_kernel<1>, ne, d_r, d_Om, part);
	else if(rd == 2) launch_per_item(ctx, edge_chi2_kernel<2>, ne, d_r, d_Om, part);
	else if(rd == 3) launch_per_item(ctx, edge_chi2_kernel<3>, ne, d_r, d_Om, part);
	else if(rd == 6) launch_per_item(ctx, edge_chi2_kernel<6>, ne, d_r, d_Om, part);
	else throw Error(SPP_E_UNSUPPORTED, "chi2: residual dimension must be 1, 2, 3 or 6");
	reduce_partials(ctx, ne);
	return fetch_scalar(ctx);
}

double edge_hessian_maxdiag(spp_ctx *ctx, int64_t ne, int rd, int d0, int d1, const double *d_J0, const double *d_J1,
	const double *d_Om)
{
	if(!ne)
		return 0;
	double *part = reserve_partials(ctx, ne);
	if(rd == 2 && d0 == 6 && d1 == 3) launch_per_item(ctx, edge_maxdiag_kernel<2, 6, 3>, ne, d_J0, d_J1, d_Om, part);
	else if(rd == 3 && d0 == 3 && d1 == 3) launch_per_item(ctx, edge_maxdiag_kernel<3, 3, 3>, ne, d_J0, d_J1, d_Om, part);
	else if(rd == 6 && d0 == 6 && d1 == 6) launch_per_item(ctx, edge_maxdiag_kernel<6, 6, 6>, ne, d_J0, d_J1, d_Om, part);
	else if(rd == 3 && d0 == 6 && d1 == 3) launch_per_item(ctx, edge_maxdiag_kernel<3, 6, 3>, ne, d_J0, d_J1, d_Om, part);
	else if(rd == 1 && d0 == 6 && d1 == 3) launch_per_item(ctx, edge_maxdiag_kernel<1, 6, 3>, ne, d_J0, d_J1, d_Om, part);
	else if(rd == 2 && d0 == 7 && d1 == 3) launch_per_item(ctx, edge_maxdiag_kernel<2, 7, 3>, ne, d_J0, d_J1, d_Om, part);
	else throw Error(SPP_E_UNSUPPORTED, "max Hessian diagonal: edge group must be (2,6,3), (3,3,3), (6,6,6), (3,6,3), (1,6,3) or (2,7,3)");
	reduce_partials(ctx, ne, true);
	return fetch_scalar(ctx);
}

double lm_gain_denominator(spp_ctx *ctx, int64_t n, const double *d_dx, const double *d_rhs, double alpha)
{
	if(!n)
		return 0;
	launch_per_item(ctx, gain_partial_kernel, n, d_dx, d_rhs, alpha, reserve_partials(ctx, n));
	reduce_partials(ctx, n);
	return fetch_scalar(ctx);
}

void se3_linearize(spp_ctx *ctx, int64_t ne, const int32_t *d_v0, const int32_t *d_v1, const double *d_poses,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se3_linearize_kernel, ne, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r);
}

double se3_update(spp_ctx *ctx, int64_t nv, double *d_poses, const double *d_dx, bool apply)
{
	if(!nv)
		return 0;
	enqueue_norm2(ctx, 6 * nv, d_dx);
	if(apply)
		launch_per_item(ctx, se3_update_kernel, nv, d_poses, d_dx);
	return fetch_scalar(ctx);
}

void ba_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, ba_linearize_kernel, no, d_cam_of, d_pt_of, d_cams, d_intr, d_pts, d_meas, d_J0, d_J1, d_r);
}

void ba_stereo_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, ba_stereo_linearize_kernel, no, d_cam_of, d_pt_of, d_cams, d_intr, d_pts, d_meas, d_J0, d_J1, d_r);
}

void ba_intrinsics_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const int32_t *d_intr_of,
	const double *d_cams, const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_J2,
	double *d_r)
{
	launch_per_item(ctx, ba_intrinsics_linearize_kernel, no, d_cam_of, d_pt_of, d_intr_of, d_cams, d_intr, d_pts, d_meas, d_J0, d_J1,
		d_J2, d_r);
}

double ba_intrinsics_update(spp_ctx *ctx, int64_t ni, double *d_intr, const int64_t *d_intr_dxoff, const double *d_dx, bool apply)
{
	if(!ni)
		return 0.0;
	ctx->geom_partial.reserve(2);
	hipLaunchKernelGGL(intrinsics_norm2_kernel, dim3(1), dim3(256), 0, ctx->stream, ni, d_intr_dxoff, d_dx, ctx->geom_partial.p);
	if(apply)
		launch_per_item(ctx, ba_update_intrinsics_kernel, ni, d_intr, d_intr_dxoff, d_dx);
	return fetch_scalar(ctx);
}

// n_dx = 0: there is no norm to copy, and the stream is synchronized all the same
double ba_update(spp_ctx *ctx, int64_t nc, double *d_cams, const int64_t *d_cam_dxoff, int64_t np, double *d_pts,
	const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, bool apply)
{
	enqueue_norm2(ctx, n_dx, d_dx);
	if(apply) {
		launch_per_item(ctx, ba_update_cams_kernel, nc, d_cams, d_cam_dxoff, d_dx);
		launch_per_item(ctx, ba_update_points_kernel, np, d_pts, d_pt_dxoff, d_dx);
	}
	if(n_dx)
		return fetch_scalar(ctx);
	SPP_HIP_CHECK(hipGetLastError());
	SPP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return 0;
}

void se2_linearize(spp_ctx *ctx, int64_t ne, const int32_t *d_v0, const int32_t *d_v1, const double *d_poses,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se2_linearize_kernel, ne, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r);
}

// returns ||dx||^2 (synchronizes the stream: the caller needs the value for the stopping test, as the
// reference does, NonlinearSolver_Lambda.h:638-650)
double se2_update(spp_ctx *ctx, int64_t nv, double *d_poses, const double *d_dx, bool apply)
{
	if(!nv)
		return 0;
	launch_per_item(ctx, se2_update_kernel, nv, d_poses, d_dx, apply ? 1 : 0, reserve_partials(ctx, nv));
	reduce_partials(ctx, nv);
	return fetch_scalar(ctx);
}

// --------------------------------------------------------------------------------------------------
// 2D landmark SLAM: 3-wide poses and 2-wide landmarks in ONE flat state laid out like eta (state and increment have
// the same layout in 2D), vertices addressed by their scalar offset. Reference (functional spec):
//   C2DJacobians::Observation2D_RangeBearing                  include/slam/2DSolverBase.h:443-496
//   CEdgePoseLandmark2D::Calculate_Jacobians_Expectation_Error include/slam/SE2_Types.h:562-573
//   CVertexPose2D::Operator_Plus (angle clamped) / CVertexLandmark2D::Operator_Plus (plain sum)  SE2_Types.h:70-74, :89
// One thread per edge; the odometry edge moves what se2_linearize_kernel moves (+ 2 x 8 B of offsets instead of 2 x 4 B
// of ids), the observation 24 + 16 B of gathered state, 16 B measurement and 16 B offsets in, 96 B out.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void se2_linearize_at_kernel(int64_t ne, const int64_t *__restrict__ off0, const int64_t *__restrict__ off1,
	const double *__restrict__ state, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	se2_linearize_edge(e, state + off0[e], state + off1[e], meas, J0, J1, r);
}

__global__ __launch_bounds__(256)
void se2_rb_linearize_kernel(int64_t ne, const int64_t *__restrict__ pose_off, const int64_t *__restrict__ lm_off,
	const double *__restrict__ state, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	const double *p = state + pose_off[e], *l = state + lm_off[e];
	const double de = l[0] - p[0], dn = l[1] - p[1], pa = p[2];
	double d = sqrt(de * de + dn * dn);
	const double hb = clamp_angle_2pi(atan2(dn, de) - pa);
	if(fabs(d) < 1e-5)
		d = 1e-5; // the floor comes BEFORE the Jacobians (2DSolverBase.h:475-476)
	const double d2 = d * d;
	r[2 * e] = meas[2 * e] - d;
	r[2 * e + 1] = clamp_angular_error_2pi(meas[2 * e + 1] - hb);
	double *a = J0 + 6 * e; // 2 x 3 column-major
	a[0] = -de / d;  a[1] = dn / d2;
	a[2] = -dn / d;  a[3] = -de / d2;
	a[4] = 0;        a[5] = -1;
	double *b = J1 + 4 * e; // 2 x 2 column-major
	b[0] = de / d;   b[1] = -dn / d2;
	b[2] = dn / d;   b[3] = de / d2;
}

__global__ __launch_bounds__(256)
void axpy1_kernel(int64_t n, double *__restrict__ x, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n)
		x[i] += dx[i];
}

__global__ __launch_bounds__(256)
void clamp_angles_kernel(int64_t na, const int64_t *__restrict__ off, double *__restrict__ x)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < na)
		x[off[i]] = clamp_angle_2pi(x[off[i]]);
}

void se2_linearize_at(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se2_linearize_at_kernel, ne, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r);
}

void se2_rb_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_pose_off, const int64_t *d_lm_off, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se2_rb_linearize_kernel, ne, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r);
}

// ||dx||^2 (two-stage sum, as se3_update) and, if apply, x += dx over the flat state, then the pose angles clamped: the sum
// is rounded once and then reduced, which is what CVertexPose2D::Operator_Plus does; landmarks keep the plain sum
double slam2d_update(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_angles,
	const int64_t *d_angle_off, bool apply)
{
	if(!n)
		return 0;
	enqueue_norm2(ctx, n, d_dx);
	if(apply) {
		launch_per_item(ctx, axpy1_kernel, n, d_state, d_dx);
		launch_per_item(ctx, clamp_angles_kernel, n_angles, d_angle_off, d_state);
	}
	return fetch_scalar(ctx);
}

// --------------------------------------------------------------------------------------------------
// 3D landmark SLAM: 6-wide poses [t | axis-angle] and 3-wide landmarks in ONE flat state laid out like eta (in 3D, too,
// state and increment have the same layout), vertices addressed by their scalar offset. Reference (functional spec):
//   C3DJacobians::Absolute_to_Relative_Landmark   e = R(a)^T (l - t)       include/slam/3DSolverBase.h:1528-1539
//   its Jacobians: forward differences (delta = 1e-9) over pose (+) d = Relative_to_Absolute(pose, d) (:807-850: t' = t +
//   R dt, R' = R exp(dr)) and over an additive landmark increment        :1602-1637
//   CEdgePoseLandmark3D::Calculate_Jacobians_Expectation_Error  r = z - e, nothing wrapped   include/slam/SE3_Types.h:568-586
//   CVertexLandmark3D::Operator_Plus (plain sum)                          SE3_Types.h:110-113
// Here analytic: e(t + R dt, R exp(dr)) = exp(dr)^T (e - dt) = e - dt - dr x e + O(d^2), so
//   d e / d dt = -I,  d e / d dr = [e]x,  d e / d l = R^T.
// One thread per observation: 6 + 3 gathered doubles, 24 B measurement, 16 B offsets in; 240 B out (J0 3 x 6, J1 3 x 3
// column-major, r 3); a wave's stores fill whole cache lines of the three outputs.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void se3_linearize_at_kernel(int64_t ne, const int64_t *__restrict__ off0, const int64_t *__restrict__ off1,
	const double *__restrict__ state, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	se3_linearize_edge(e, state + off0[e], state + off1[e], meas, J0, J1, r);
}

__global__ __launch_bounds__(256)
void se3_xyz_linearize_kernel(int64_t ne, const int64_t *__restrict__ pose_off, const int64_t *__restrict__ lm_off,
	const double *__restrict__ state, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	const double *p = state + pose_off[e], *l = state + lm_off[e], *z = meas + 3 * e;
	double R[9];
	axis_angle_to_rot(p + 3, R);
	const double d0 = l[0] - p[0], d1 = l[1] - p[1], d2 = l[2] - p[2];
	const double e0 = R[0] * d0 + R[3] * d1 + R[6] * d2, e1 = R[1] * d0 + R[4] * d1 + R[7] * d2,
		e2 = R[2] * d0 + R[5] * d1 + R[8] * d2; // R^T (l - t)
	double *ro = r + 3 * e;
	ro[0] = z[0] - e0; ro[1] = z[1] - e1; ro[2] = z[2] - e2;
	double *a = J0 + 18 * e; // [ -I | [e]x ], element (row, col) at row + 3 col
	a[0] = -1; a[1] = 0;  a[2] = 0;
	a[3] = 0;  a[4] = -1; a[5] = 0;
	a[6] = 0;  a[7] = 0;  a[8] = -1;
	a[9] = 0;    a[10] = e2;  a[11] = -e1;
	a[12] = -e2; a[13] = 0;   a[14] = e0;
	a[15] = e1;  a[16] = -e0; a[17] = 0;
	double *b = J1 + 9 * e; // R^T column-major = R row-major
#pragma unroll
	for(int q = 0; q < 9; ++ q)
		b[q] = R[q];
}

// the listed poses' new values into tmp (6 each), from the state BEFORE the plain sum below touches it
__global__ __launch_bounds__(256)
void slam3d_pose_plus_kernel(int64_t np, const int64_t *__restrict__ pose_off, const double *__restrict__ x,
	const double *__restrict__ dx, double *__restrict__ tmp)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= np)
		return;
	se3_plus(x + pose_off[i], dx + pose_off[i], tmp + 6 * i);
}

__global__ __launch_bounds__(256)
void slam3d_pose_store_kernel(int64_t np, const int64_t *__restrict__ pose_off, const double *__restrict__ tmp,
	double *__restrict__ x)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // one thread per pose entry
	if(i < 6 * np)
		x[pose_off[i / 6] + i % 6] = tmp[i];
}

void se3_linearize_at(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se3_linearize_at_kernel, ne, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r);
}

void se3_xyz_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_pose_off, const int64_t *d_lm_off, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, se3_xyz_linearize_kernel, ne, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r);
}

// ||dx||^2 over the flat increment (two-stage sum, as se3_update) and, if apply: the listed poses composed (se3_plus on the
// old state, parked behind the partial sums), x += dx everywhere -- the landmarks' CVertexLandmark3D::Operator_Plus --, then
// the composed poses written over their six entries
double slam3d_update(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_poses,
	const int64_t *d_pose_off, bool apply)
{
	if(!n)
		return 0;
	enqueue_norm2(ctx, n, d_dx, apply ? (size_t)(6 * n_poses) : 0);
	if(apply) {
		double *tmp = ctx->geom_partial.p + 1 + n_workgroups(n);
		launch_per_item(ctx, slam3d_pose_plus_kernel, n_poses, d_pose_off, d_state, d_dx, tmp);
		launch_per_item(ctx, axpy1_kernel, n, d_state, d_dx);
		launch_over(ctx, slam3d_pose_store_kernel, 6 * n_poses, n_poses, d_pose_off, tmp, d_state);
	}
	return fetch_scalar(ctx);
}

// --------------------------------------------------------------------------------------------------
// Range-only constant-velocity SLAM (ROCV): 6-wide receivers [p | v] and 3-wide transmitters in ONE flat state laid out
// like eta, vertices addressed by their scalar offset; both vertex types add their increment plainly
// (CVertexPositionVelocity3D::Operator_Plus, include/slam/ROCV_Types.h:60-63; CVertexLandmark3D), so the update is
// slam2d_update with no angles. Reference (functional spec):
//   CEdgePosVel_Landmark3D<false>::Calculate_Jacobians_Expectation_Error   ROCV_Types.h:163-205
//     e = |p - l|, r = z - e, J0 = [(p - l)^T / e | 0 0 0], J1 = -J0[0:3]. The reference divides by the square root of the
//     EXPANDED polynomial lx^2 - 2 lx x + x^2 + ..., which cancels when p is near l; here e is formed from the differences
//     (as its own expectation is, :200). At e = 0 the reference divides 0 by 0; here both Jacobians are exact zeros and
//     r = z: nothing is divided by e.
//   CEdgeConstVelocity3D<false>::Calculate_Jacobians_Expectation_Error     ROCV_Types.h:543-614
//     expectation = (p0 + v0 dt, v0), r = -(x1 - expectation) (the reversed sign of :608), J0 = -[I, dt I; 0, I], J1 = I,
//     in the layout of the (6,6,6) group.
// One thread per edge. Range: 6 gathered doubles, 8 B measurement, 16 B offsets in; 80 B out (J0 1 x 6, J1 1 x 3, r 1).
// Constant velocity: 12 gathered doubles, 8 B dt, 16 B offsets in; 624 B out, all but 3 + 6 of them constants.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void rocv_range_linearize_kernel(int64_t ne, const int64_t *__restrict__ recv_off, const int64_t *__restrict__ lm_off,
	const double *__restrict__ state, const double *__restrict__ meas, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	const double *p = state + recv_off[e], *l = state + lm_off[e];
	const double d0 = p[0] - l[0], d1 = p[1] - l[1], d2 = p[2] - l[2];
	const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
	const double u0 = dist > 0 ? d0 / dist : 0.0, u1 = dist > 0 ? d1 / dist : 0.0, u2 = dist > 0 ? d2 / dist : 0.0;
	r[e] = meas[e] - dist;
	double *a = J0 + 6 * e;
	a[0] = u0; a[1] = u1; a[2] = u2; a[3] = 0; a[4] = 0; a[5] = 0;
	double *b = J1 + 3 * e;
	b[0] = -u0; b[1] = -u1; b[2] = -u2;
}

__global__ __launch_bounds__(256)
void rocv_cv_linearize_kernel(int64_t ne, const int64_t *__restrict__ off0, const int64_t *__restrict__ off1,
	const double *__restrict__ state, const double *__restrict__ dts, double *__restrict__ J0,
	double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ne)
		return;
	const double *x0 = state + off0[e], *x1 = state + off1[e];
	const double dt = dts[e];
	double *ro = r + 6 * e, *a = J0 + 36 * e, *b = J1 + 36 * e;
#pragma unroll
	for(int i = 0; i < 3; ++ i) {
		ro[i] = -(x1[i] - (x0[i] + x0[3 + i] * dt));
		ro[3 + i] = -(x1[3 + i] - x0[3 + i]);
	}
#pragma unroll
	for(int c = 0; c < 6; ++ c)
#pragma unroll
		for(int i = 0; i < 6; ++ i) { // element (row i, column c) at i + 6 c
			a[i + 6 * c] = (i == c) ? -1.0 : (c == i + 3) ? -dt : 0.0;
			b[i + 6 * c] = (i == c) ? 1.0 : 0.0;
		}
}

void rocv_range_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_recv_off, const int64_t *d_lm_off, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, rocv_range_linearize_kernel, ne, d_recv_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r);
}

void rocv_cv_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_dt, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, rocv_cv_linearize_kernel, ne, d_off0, d_off1, d_state, d_dt, d_J0, d_J1, d_r);
}

// --------------------------------------------------------------------------------------------------
// Sim(3) bundle adjustment: the edge CEdgeP2C_XYZ_Sim3_G (include/slam/Sim3_Types.h:492-595) between a point CVertexXYZ and
// a camera CVertexCamSim3, a 7-vector v = [t | w | s] of sim(3) with 5 constant intrinsics. Reference (functional spec):
//   CSim3Jacobians::t_Exp                include/slam/Sim3SolverBase.h:3829-3905   T = Exp(v) = (R, tau, sigma):
//       R = exp([w]x), sigma = e^s, tau = V t, V = a I + b [w]x + c [w]x^2
//   CSim3Jacobians::v_Log                :3740-3819 (the inverse; solves V t = tau by a Householder QR)
//   CSim3Jacobians::Project_P2C_XYZ      :630-681   x = T^-1 X = e^-s R^T (X - tau), p - c = (fx x0/x2, fy x1/x2),
//       k = intr[4] / (0.5 fx fy) -- the PRODUCT of the focal lengths --, uv = c + (1 + |p - c|^2 k)(p - c); r = z - uv
//   its Jacobians                         :1043-1062 forward differences (delta = 1e-9) over Relative_to_Absolute (:435-452),
//       the POST-multiplicative camera increment T Exp(d), and over an additive point increment
// With theta = |w| and z = s + i theta the coefficients are a = phi(s), b = Im phi(z) / theta, c = (a - Re phi(z)) / theta^2,
// phi(z) = (e^z - 1) / z. The reference evaluates them in four cells (|s|, theta against 1e-6), whose closed forms lose
// digits to cancellation just above the thresholds; here (sim3_abc)
//   |z|^2 < 1   the Taylor series b = sum p_n / (n + 1)!, c = sum q_n / (n + 1)! with p_n = Im z^n / theta,
//               q_n = (s^n - Re z^n) / theta^2 by the recurrence p' = s p + s^n - theta^2 q, q' = s q + p (no division)
//   otherwise   b = (s (E S - a) + E theta^2 C) / |z|^2, c = (a - E (S - s C)) / |z|^2 with E = e^s, S = sin(theta) / theta,
//               C = (1 - cos(theta)) / theta^2 (S, C by two terms below theta = 1e-4): nothing is divided by theta
// and a = expm1(s) / s. Jacobians analytic: x (T Exp(d)) = Exp(-d) x = x - dt - dw x x - ds x to first order, so
//   d x / d d = [-I | [x]x | -x],  d x / d X = e^-s R^T,  J = P d x / d ., P = d uv / d x (2 x 3, as in ba_p2c_edge).
// P x = 0 identically (the projection does not see the scale of the camera frame): the scale column of J0 is written as
// exact zeros. Nothing is divided by |p - c|: a point on the optical axis gives finite Jacobians.
// Log: V^-1 = (1 / a) I - (b / D) [w]x + ((b^2 - A c) / (a D)) [w]x^2, A = a - c theta^2, D = A^2 + theta^2 b^2 = |phi(z)|^2,
// in closed form ([w]x^3 = -theta^2 [w]x) instead of the reference's QR.
// One thread per observation: 12 + 3 gathered doubles + 16 B in, 176 B out (J0 2x7, J1 2x3 column-major, r).
// --------------------------------------------------------------------------------------------------
constexpr int SIM3_SERIES_TERMS = 24; // n |z|^(n-1) / (n + 1)! < 1e-19 from n = 21 on, |z| < 1

// S = sin(theta) / theta, C = (1 - cos(theta)) / theta^2 and the half-angle pair (cos(theta / 2), sin(theta / 2) / theta)
__device__ __forceinline__ void sim3_sinc(double th, double *S, double *C, double *ch, double *sh_over)
{
	if(th < 1e-4) {
		const double th2 = th * th;
		*S = 1.0 - th2 * (1.0 / 6.0);
		*C = 0.5 - th2 * (1.0 / 24.0);
		*ch = 1.0 - th2 * 0.125;
		*sh_over = 0.5 - th2 * (1.0 / 48.0);
	} else {
		double sh, c;
		sincos(0.5 * th, &sh, &c);
		const double so = sh / th;
		*S = 2.0 * so * c;
		*C = 2.0 * so * so;
		*ch = c;
		*sh_over = so;
	}
}

// a, b, c of V at (s, theta); E = e^s, S and C as above
__device__ __forceinline__ void sim3_abc(double s, double th, double E, double S, double C, double *a, double *b, double *c)
{
	const double th2 = th * th, z2 = s * s + th2;
	const double av = (s == 0.0) ? 1.0 : expm1(s) / s;
	*a = av;
	if(z2 < 1.0) {
		double p = 0, q = 0, sn = 1, f = 1, bs = 0, cs = 0;
		for(int n = 0; n < SIM3_SERIES_TERMS; ++ n) {
			f /= (double)(n + 1);
			bs += p * f;
			cs += q * f;
			const double pn = s * p + sn - th2 * q;
			q = s * q + p;
			p = pn;
			sn *= s;
		}
		*b = bs;
		*c = cs;
	} else {
		*b = (s * (E * S - av) + E * th2 * C) / z2;
		*c = (av - E * (S - s * C)) / z2;
	}
}

// T = Exp(v): R row-major, tau, E = e^s; q (may be null) <- the unit quaternion (w, x, y, z) of R with w >= 0
__device__ __forceinline__ void sim3_exp(const double *v, double *R, double *tau, double *E_out, double *q)
{
	const double x = v[3], y = v[4], z = v[5], s = v[6];
	const double th = sqrt(x * x + y * y + z * z), E = exp(s);
	double S, C, ch, so, a, b, c;
	sim3_sinc(th, &S, &C, &ch, &so);
	sim3_abc(s, th, E, S, C, &a, &b, &c);
	R[0] = 1 - C * (y * y + z * z); R[1] = C * x * y - S * z;       R[2] = C * x * z + S * y;
	R[3] = C * x * y + S * z;       R[4] = 1 - C * (x * x + z * z); R[5] = C * y * z - S * x;
	R[6] = C * x * z - S * y;       R[7] = C * y * z + S * x;       R[8] = 1 - C * (x * x + y * y);
	const double t0 = v[0], t1 = v[1], t2 = v[2];
	const double c0 = y * t2 - z * t1, c1 = z * t0 - x * t2, c2 = x * t1 - y * t0;       // w x t
	const double d0 = y * c2 - z * c1, d1 = z * c0 - x * c2, d2 = x * c1 - y * c0;       // w x (w x t)
	tau[0] = a * t0 + b * c0 + c * d0;
	tau[1] = a * t1 + b * c1 + c * d1;
	tau[2] = a * t2 + b * c2 + c * d2;
	*E_out = E;
	if(q) {
		const double sg = (ch < 0) ? -1.0 : 1.0;
		q[0] = sg * ch; q[1] = sg * so * x; q[2] = sg * so * y; q[3] = sg * so * z;
	}
}

__global__ __launch_bounds__(256)
void sim3_ba_linearize_kernel(int64_t no, const int32_t *__restrict__ cam_of, const int32_t *__restrict__ pt_of,
	const double *__restrict__ cams, const double *__restrict__ intr, const double *__restrict__ pts,
	const double *__restrict__ meas, double *__restrict__ J0, double *__restrict__ J1, double *__restrict__ r)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= no)
		return;
	const double *cam = cams + 7 * (int64_t)cam_of[e], *in = intr + 5 * (int64_t)cam_of[e], *X = pts + 3 * (int64_t)pt_of[e];
	double R[9], tau[3], E;
	sim3_exp(cam, R, tau, &E, nullptr);
	const double iE = 1.0 / E, y0 = X[0] - tau[0], y1 = X[1] - tau[1], y2 = X[2] - tau[2];
	const double x0 = iE * (R[0] * y0 + R[3] * y1 + R[6] * y2); // e^-s R^T (X - tau)
	const double x1 = iE * (R[1] * y0 + R[4] * y1 + R[7] * y2);
	const double x2 = iE * (R[2] * y0 + R[5] * y1 + R[8] * y2);
	const double fx = in[0], fy = in[1], k = in[4] / (0.5 * (fx * fy));
	const double iz = 1.0 / x2, d0 = fx * x0 * iz, d1 = fy * x1 * iz, r2 = d0 * d0 + d1 * d1, g = 1.0 + r2 * k;
	r[2 * e] = meas[2 * e] - (in[2] + g * d0);
	r[2 * e + 1] = meas[2 * e + 1] - (in[3] + g * d1);
	// P = d uv / d x (2 x 3) = ((g) I + 2 k d d^T) [fx/z 0 -fx x0/z^2; 0 fy/z -fy x1/z^2]
	const double D00 = g + 2 * k * d0 * d0, D01 = 2 * k * d0 * d1, D11 = g + 2 * k * d1 * d1;
	const double a0 = fx * iz, a2 = -fx * x0 * iz * iz, b1 = fy * iz, b2 = -fy * x1 * iz * iz;
	const double P[6] = {D00 * a0, D01 * b1, D00 * a2 + D01 * b2,   // row 0
	                     D01 * a0, D11 * b1, D01 * a2 + D11 * b2};  // row 1
	double *a = J0 + 14 * e, *b = J1 + 6 * e;
#pragma unroll
	for(int i = 0; i < 2; ++ i) {
		const double p0 = P[3 * i], p1 = P[3 * i + 1], p2 = P[3 * i + 2];
		a[i] = -p0; a[2 + i] = -p1; a[4 + i] = -p2;                    // d / d dt = -P
		a[6 + i] = p1 * x2 - p2 * x1;                                  // d / d dw = P [x]x
		a[8 + i] = p2 * x0 - p0 * x2;
		a[10 + i] = p0 * x1 - p1 * x0;
		a[12 + i] = 0.0;                                               // d / d ds = -P x = 0
#pragma unroll
		for(int j = 0; j < 3; ++ j)                                    // d / d X = P e^-s R^T
			b[2 * j + i] = iE * (p0 * R[3 * j] + p1 * R[3 * j + 1] + p2 * R[3 * j + 2]);
	}
}

// camera <- Log(Exp(camera) Exp(d)) (CVertexCamSim3::Operator_Plus = Relative_to_Absolute, Sim3SolverBase.h:435-452):
// (R1, tau1, E1)(R2, tau2, E2) = (R1 R2, tau1 + E1 R1 tau2, E1 E2), rotations composed as unit quaternions, s = s1 + s2
__global__ __launch_bounds__(256)
void sim3_update_cams_kernel(int64_t nc, double *__restrict__ cams, const int64_t *__restrict__ dxoff, const double *__restrict__ dx)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= nc)
		return;
	double *cam = cams + 7 * i;
	const double *d = dx + dxoff[i];
	double v1[7], v2[7];
#pragma unroll
	for(int j = 0; j < 7; ++ j) {
		v1[j] = cam[j];
		v2[j] = d[j];
	}
	double R1[9], R2[9], t1[3], t2[3], E1, E2, q1[4], q2[4], q[4], w[3];
	sim3_exp(v1, R1, t1, &E1, q1);
	sim3_exp(v2, R2, t2, &E2, q2);
	const double tau0 = t1[0] + E1 * (R1[0] * t2[0] + R1[1] * t2[1] + R1[2] * t2[2]);
	const double tau1 = t1[1] + E1 * (R1[3] * t2[0] + R1[4] * t2[1] + R1[5] * t2[2]);
	const double tau2 = t1[2] + E1 * (R1[6] * t2[0] + R1[7] * t2[1] + R1[8] * t2[2]);
	quat_mul(q1, q2, q);
	quat_to_aa(q[0], q[1], q[2], q[3], w);
	const double s = v1[6] + v2[6];
	const double x = w[0], y = w[1], z = w[2], th2 = x * x + y * y + z * z, th = sqrt(th2);
	double S, C, ch, so, a, b, c;
	sim3_sinc(th, &S, &C, &ch, &so);
	sim3_abc(s, th, exp(s), S, C, &a, &b, &c);
	const double A = a - c * th2, D = A * A + th2 * b * b;
	const double al = 1.0 / a, be = -b / D, ga = (b * b - A * c) / (a * D);
	const double c0 = y * tau2 - z * tau1, c1 = z * tau0 - x * tau2, c2 = x * tau1 - y * tau0;   // w x tau
	const double e0 = y * c2 - z * c1, e1 = z * c0 - x * c2, e2 = x * c1 - y * c0;               // w x (w x tau)
	cam[0] = al * tau0 + be * c0 + ga * e0;
	cam[1] = al * tau1 + be * c1 + ga * e1;
	cam[2] = al * tau2 + be * c2 + ga * e2;
	cam[3] = x; cam[4] = y; cam[5] = z;
	cam[6] = s;
}

void sim3_ba_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r)
{
	launch_per_item(ctx, sim3_ba_linearize_kernel, no, d_cam_of, d_pt_of, d_cams, d_intr, d_pts, d_meas, d_J0, d_J1, d_r);
}

// (the shape of ba_update: the norm over all of dx, cameras through Log(Exp Exp), points as plain sums)
double sim3_update(spp_ctx *ctx, int64_t nc, double *d_cams, const int64_t *d_cam_dxoff, int64_t np, double *d_pts,
	const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, bool apply)
{
	enqueue_norm2(ctx, n_dx, d_dx);
	if(apply) {
		launch_per_item(ctx, sim3_update_cams_kernel, nc, d_cams, d_cam_dxoff, d_dx);
		launch_per_item(ctx, ba_update_points_kernel, np, d_pts, d_pt_dxoff, d_dx);
	}
	if(n_dx)
		return fetch_scalar(ctx);
	SPP_HIP_CHECK(hipGetLastError());
	SPP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return 0;
}

} // namespace spp
