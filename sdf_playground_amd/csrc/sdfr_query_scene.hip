// sdfr_query_scene.hip -- the query kernels (k_query_points, k_query_rays: sdfr_query_kernel.h) of ONE scene, compiled
// once per scene with -DSDFR_SCENE=<index> and the scene's code-generation options (sdf_playground_amd/buildlib.py), like
// sdfr_kernels_scene.hip.  They live in a unit of their own: a second caller of the shared inline stages in the pixel kernels'
// unit could change the inliner's decisions there, and with them k_pixel's code.
//
// Plain IEEE sqrt / reciprocal / constant division (SDFR_SAFE_MATH, sdfr_math.h), as scenes compiled at run time get them: the
// fast forms of the pixel kernels are exact only on the domains the render workloads are verified on, and a query takes any
// point and any ray -- a ray that starts below the floor already makes the normal's sum of squares overflow to +inf, where the
// fast square root gives NaN and the driver's normalize 0.  On those domains both forms give the same bits.
#define SDFR_SAFE_MATH 1
#include "sdfr_kernels.h"
#include "sdfr_perpixel.h"
#include "sdfr_query_kernel.h"

#ifndef SDFR_SCENE
#error "compile with -DSDFR_SCENE=<scene index, sdfr_perpixel.h>"
#endif

namespace sdfr {

template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_points(QueryKernelArgs a)
{
	query_points_kernel<Scene, DBG>(a);
}

// rays and picks (rays made from pixels)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_rays(QueryKernelArgs a)
{
	query_rays_kernel<Scene, DBG>(a);
}

template <class Scene, bool DBG>
static hipError_t run_query(const FrameU &U, const QueryArgs &q, hipStream_t stream)
{
	const uint32_t blocks = ((uint32_t)q.n + SDFR_PIXEL_BLOCK - 1u) / SDFR_PIXEL_BLOCK;
	QueryKernelArgs a;
	a.U = U;
	a.q = q;
	if (q.kind == QUERY_POINTS)
		hipLaunchKernelGGL((k_query_points<Scene, DBG>), dim3(blocks), dim3(SDFR_PIXEL_BLOCK), 0, stream, a);
	else
		hipLaunchKernelGGL((k_query_rays<Scene, DBG>), dim3(blocks), dim3(SDFR_PIXEL_BLOCK), 0, stream, a);
	return hipGetLastError();
}

#define SDFR_CAT2(a, b) a##b
#define SDFR_CAT(a, b) SDFR_CAT2(a, b)
using UnitScene = SceneAt<SDFR_SCENE>::type;

hipError_t SDFR_CAT(launch_query_scene, SDFR_SCENE)(const FrameU &U, const QueryArgs &q, hipStream_t stream)
{
	return frame_needs_debug(U) ? run_query<UnitScene, true>(U, q, stream) : run_query<UnitScene, false>(U, q, stream);
}

} // namespace sdfr
