// sdfr_query_scene.hip -- the query kernels (k_query_points, k_query_rays, k_query_lattice, k_query_surfaces, k_query_occlusion, k_query_lighting, k_bake_atlas, k_mesh_sharp, k_query_slices, k_query_spans, k_query_measure: sdfr_query_kernel.h) of ONE scene, compiled
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

// the distance query over a lattice of points made from their indices (sdfr_mesh_extract)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_lattice(LatticeKernelArgs a)
{
	query_lattice_kernel<Scene, DBG>(a);
}

// the surface under rays, pixels, a whole frame or towards a mesh's vertices (sdfr_surface.h)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_surfaces(QueryKernelArgs a)
{
	query_surfaces_kernel<Scene, DBG>(a);
}

// ambient occlusion at points or hits: a wave per item (sdfr_occlusion.h)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_occlusion(QueryKernelArgs a)
{
	query_occlusion_kernel<Scene, DBG>(a);
}

// direct lighting at the hits of rays, pixels, a whole frame or a mesh's vertices (sdfr_lighting.h)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_lighting(QueryKernelArgs a)
{
	query_lighting_kernel<Scene, DBG>(a);
}

// the atlas bake: a texel of a mesh's texture atlas per lane (sdfr_atlas.h)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_bake_atlas(AtlasKernelArgs a)
{
	atlas_bake_kernel<Scene, DBG>(a);
}

// the sharp vertices of a mesh: 16 lanes per vertex (sdfr_mesh_sharp.h; sdfr_mesh_extract_sharp)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_mesh_sharp(MeshSharpKernelArgs a)
{
	mesh_sharp_kernel<Scene, DBG>(a);
}

// the distance query over a stack of plane lattices made from their indices (sdfr_slice_extract)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_slices(SliceKernelArgs a)
{
	query_slices_kernel<Scene, DBG>(a);
}

// the intervals of rays, pixels' rays and mesh rays that lie inside the solid (sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_spans(SpanKernelArgs a)
{
	query_spans_kernel<Scene, DBG>(a);
}

// the moments of the solid over a bundle of parallel columns (sdfr_measure)
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_query_measure(MeasureKernelArgs a)
{
	query_measure_kernel<Scene, DBG>(a);
}

using UnitScene = SceneAt<SDFR_SCENE>::type;

// what this unit exports (scene_query_kernels, launch_query: sdfr_kernels.hip)
const QueryKernels *SDFR_CAT(scene_query_kernels_, SDFR_SCENE)()
{
	// (the debug variants first: the order the kernels are first named in is their order in the unit's code object, kept as it was)
	static const QueryKernels k = [] {
		QueryKernels q = {};
		q.k[QUERY_KERNEL_POINTS][1].kernel = (const void *)k_query_points<UnitScene, true>;
		q.k[QUERY_KERNEL_RAYS][1].kernel = (const void *)k_query_rays<UnitScene, true>;
		q.k[QUERY_KERNEL_POINTS][0].kernel = (const void *)k_query_points<UnitScene, false>;
		q.k[QUERY_KERNEL_RAYS][0].kernel = (const void *)k_query_rays<UnitScene, false>;
		q.k[QUERY_KERNEL_LATTICE][1].kernel = (const void *)k_query_lattice<UnitScene, true>;
		q.k[QUERY_KERNEL_LATTICE][0].kernel = (const void *)k_query_lattice<UnitScene, false>;
		q.k[QUERY_KERNEL_SURFACES][1].kernel = (const void *)k_query_surfaces<UnitScene, true>;
		q.k[QUERY_KERNEL_SURFACES][0].kernel = (const void *)k_query_surfaces<UnitScene, false>;
		q.k[QUERY_KERNEL_OCCLUSION][1].kernel = (const void *)k_query_occlusion<UnitScene, true>;
		q.k[QUERY_KERNEL_OCCLUSION][0].kernel = (const void *)k_query_occlusion<UnitScene, false>;
		q.k[QUERY_KERNEL_LIGHTING][1].kernel = (const void *)k_query_lighting<UnitScene, true>;
		q.k[QUERY_KERNEL_LIGHTING][0].kernel = (const void *)k_query_lighting<UnitScene, false>;
		q.k[QUERY_KERNEL_ATLAS][1].kernel = (const void *)k_bake_atlas<UnitScene, true>;
		q.k[QUERY_KERNEL_ATLAS][0].kernel = (const void *)k_bake_atlas<UnitScene, false>;
		q.k[QUERY_KERNEL_MESH_SHARP][1].kernel = (const void *)k_mesh_sharp<UnitScene, true>;
		q.k[QUERY_KERNEL_MESH_SHARP][0].kernel = (const void *)k_mesh_sharp<UnitScene, false>;
		q.k[QUERY_KERNEL_SLICES][1].kernel = (const void *)k_query_slices<UnitScene, true>;
		q.k[QUERY_KERNEL_SLICES][0].kernel = (const void *)k_query_slices<UnitScene, false>;
		q.k[QUERY_KERNEL_SPANS][1].kernel = (const void *)k_query_spans<UnitScene, true>;
		q.k[QUERY_KERNEL_SPANS][0].kernel = (const void *)k_query_spans<UnitScene, false>;
		q.k[QUERY_KERNEL_MEASURE][1].kernel = (const void *)k_query_measure<UnitScene, true>;
		q.k[QUERY_KERNEL_MEASURE][0].kernel = (const void *)k_query_measure<UnitScene, false>;
		return q;
	}();
	return &k;
}

} // namespace sdfr
