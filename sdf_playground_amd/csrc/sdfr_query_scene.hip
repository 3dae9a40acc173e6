// sdfr_query_scene.hip -- the query kernels (k_<stem> of every kind of SDFR_FOR_EACH_QUERY_KERNEL, sdfr_query_args.h; the bodies:
// sdfr_query_kernel.h) of ONE scene, compiled once per scene with -DSDFR_SCENE=<index> and the scene's code-generation options (sdf_playground_amd/buildlib.py), like
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

// k_<stem> of every kind of the list (sdfr_query_args.h): the kind's body (sdfr_query_kernel.h) as a kernel of one by-value argument
#define SDFR_QUERY_KERNEL(kind, stem, body, args) \
	template <class Scene, bool DBG> \
	__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_##stem(SceneKernelArgs<args> a) \
	{ \
		body<Scene, DBG>(a); \
	}
SDFR_FOR_EACH_QUERY_KERNEL(SDFR_QUERY_KERNEL)
#undef SDFR_QUERY_KERNEL

using UnitScene = SceneAt<SDFR_SCENE>::type;

// what this unit exports (scene_query_kernels, launch_query: sdfr_kernels.hip)
const QueryKernels *SDFR_CAT(scene_query_kernels_, SDFR_SCENE)()
{
	// The order the kernels are first named in is their order in the unit's code object, kept as it was when the unit had two kinds:
	// the debug variants of points and rays first, then every kind of the list, debug before plain.
	static const QueryKernels k = [] {
		QueryKernels q = {};
		q.k[QUERY_KERNEL_POINTS][1].kernel = (const void *)k_query_points<UnitScene, true>;
		q.k[QUERY_KERNEL_RAYS][1].kernel = (const void *)k_query_rays<UnitScene, true>;
#define SDFR_QUERY_KERNEL(kind, stem, body, args) \
	q.k[QUERY_KERNEL_##kind][1].kernel = (const void *)k_##stem<UnitScene, true>; \
	q.k[QUERY_KERNEL_##kind][0].kernel = (const void *)k_##stem<UnitScene, false>;
		SDFR_FOR_EACH_QUERY_KERNEL(SDFR_QUERY_KERNEL)
#undef SDFR_QUERY_KERNEL
		return q;
	}();
	return &k;
}

} // namespace sdfr
