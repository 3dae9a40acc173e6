/* sdfr.h -- C ABI of the MI355X-native SDF raymarch renderer (libsdfr.so).
 *
 * This is the drop-in boundary for ONE hot path of Gotbread/sdf-playground: the SDF render
 * stage `class SDFRenderer` (Engine/SDFRenderer.h:17-44), i.e. the per-pixel raymarch loop
 * of Engine/shader/pshader_sdf.hlsl.  Each entry point names the reference interface it
 * replaces.  Plain C types only; no torch, no C++ types.
 *
 * Conventions
 *   - every call returns an sdfr_status (0 = ok, < 0 = error); sdfr_last_error() gives text.
 *     The reference returns bool and pops a MessageBox (Util.cpp:61-69); nothing here aborts.
 *   - a handle is bound to one GPU and one HIP stream; calls on one handle are not
 *     thread-safe (the reference is single-threaded, Application.cpp:65-95).
 *   - sdfr_render* enqueue work on the handle's stream and return; sdfr_sync waits.
 *   - images are row-major, row 0 = top row, 4 channels interleaved; alpha is the
 *     tone-mapping flag in {0, 1} (pshader_sdf.hlsl:636-638), not coverage.
 */
#ifndef SDFR_H
#define SDFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdfr_renderer sdfr_renderer;

typedef enum sdfr_status
{
	SDFR_OK = 0,
	SDFR_ERR_INVALID_ARGUMENT = -1,
	SDFR_ERR_UNKNOWN_SCENE = -2,
	SDFR_ERR_UNKNOWN_VARIABLE = -3, /* value ignored, like ShaderVariableManager::setValue (ShaderUtil.cpp:234-240) */
	SDFR_ERR_NO_SCENE = -4,         /* render without a loaded scene: SDFRenderer::render returns false (SDFRenderer.cpp:70-73) */
	SDFR_ERR_HIP = -5,
	SDFR_ERR_NO_DEVICE = -6,
	SDFR_ERR_COMPILE = -7, /* a run-time scene does not compile: sdfr_last_error holds the compiler's messages */
	SDFR_ERR_COMM = -8,    /* RCCL could not be loaded, or one of its calls failed: sdfr_comm_last_error / sdfr_last_error */
	SDFR_ERR_INTERNAL = -9 /* a C++ exception (out of memory, ...) was caught at the C boundary: sdfr_last_error has its words; never an abort */
} sdfr_status;

/* ---- lifetime: SDFRenderer::init(Graphics&) (SDFRenderer.cpp:9-25) ----------------------- */
int sdfr_create(int device_ordinal, sdfr_renderer **out);
void sdfr_destroy(sdfr_renderer *r);
const char *sdfr_last_error(const sdfr_renderer *r);
/* work is enqueued on this hipStream_t (NULL = the default stream) */
int sdfr_set_stream(sdfr_renderer *r, void *hip_stream);

/* ---- scene selection: SceneManager list (SceneManager.cpp:142-158) + Application::loadScene
 *      (Application.cpp:318-322) + SDFRenderer::initShader (SDFRenderer.cpp:27-53).
 *      Names are the reference's file stems without "sdf_scene_". ------------------------------ */
int sdfr_scene_count(void);
const char *sdfr_scene_name(int index);
/* besides the listed names: "debug_materials", the library's own diagnostic scene (four objects wearing
 * the driver's MATERIAL_ITER / PLAIN / NORMAL1 / NORMAL2 views, pshader_sdf.hlsl:430-455, which no
 * reference scene emits; not part of the reference's scene list, hence not counted above), and "normal_test",
 * a scene with a map_normal callback (sdf_structs.hlsl:39-52: its own normal on one object, a wider
 * normal_sample_dist -- rounded corners -- on two others), which every scene of the reference leaves empty */
int sdfr_load_scene(sdfr_renderer *r, const char *name);
const char *sdfr_current_scene(const sdfr_renderer *r);
/* Compile a scene from source text at run time -- the reference's edit-and-reload workflow
 * (SceneManager.cpp:102-133 re-runs SDFRenderer::initShader -> D3DCompile when a scene file
 * changes).  `source` is HIP C++ defining `struct Scene` with the scene interface of
 * sdf_playground_amd/scenes/README.md (the reference's map / map_light / map_background split
 * into dist / material / light / background); VAR_<name>(min = .., max = .., ..) tags in the text
 * declare variables exactly as in the reference's .hlsl scenes (ShaderUtil.cpp:122-191).  On
 * SDFR_ERR_COMPILE the previously loaded scene stays active, as in the reference
 * (SceneManager.cpp:118-127).  Needs libhiprtc.so and the kernel headers (csrc/ beside the
 * library, or $SDFR_JIT_INCLUDE). */
int sdfr_load_scene_source(sdfr_renderer *r, const char *name, const char *source);
/* Same compilation without a device or a handle (build machines, editors): SDFR_OK, or
 * SDFR_ERR_COMPILE / SDFR_ERR_INVALID_ARGUMENT with the messages in `log`.  arch: "gfx950" (NULL = that). */
int sdfr_check_scene_source(const char *source, const char *arch, char *log, size_t log_bytes);

/* The same for a scene IN THE REFERENCE'S OWN DIALECT: the text of an .hlsl scene file as Application::loadScene substitutes
 * it for "sdf_scene.hlsl" (Application.cpp:229,320; pshader_sdf.hlsl:84) -- the four callbacks map / map_normal / map_light /
 * map_background with their HLSL signatures (sdf_structs.hlsl), the OBJECT / OBJECT_TRANSPARENT / MATERIAL macros
 * (pshader_sdf.hlsl:79-81), float2/3/4 with swizzles, the intrinsics, the shader libraries under their own names
 * (sdSphere ... turbulence), the frame globals (stime, eye, ...), VAR_ tags.  The 22 scene files of the reference load as
 * they are (their `#include "sdf_*.hlsl"` lines are dropped: the libraries are this library's).  The text is compiled as
 * the body of a C++ class after a short textual pass (csrc/sdfr_hlsl.h, sdfr_hlsl.cpp); plain IEEE arithmetic, like every
 * run-time scene.  Not supported: snoise(float2) / snoise(float4), HLSL objects that have no meaning here (textures,
 * samplers, semantics).  sdfr_translate_scene_hlsl returns the generated C++ (bytes needed incl. the terminator; `out` may
 * be NULL) -- for inspection and for compiling a scene with a host compiler. */
int sdfr_load_scene_hlsl(sdfr_renderer *r, const char *name, const char *hlsl_source);
int sdfr_check_scene_hlsl(const char *hlsl_source, const char *arch, char *log, size_t log_bytes);
int sdfr_translate_scene_hlsl(const char *hlsl_source, char *out, size_t out_bytes);

/* ---- parameter surface 1: shader variables = SDFRenderer::getVariableMap()
 *      (ShaderVariable.h:6-12; ShaderUtil.cpp:122-267).  Index order = std::map order
 *      (lexicographic by name), which is also the reference's constant-buffer order. --------- */
typedef struct sdfr_variable
{
	char name[48];
	float minval, maxval, start, step;
	float value;
} sdfr_variable;
int sdfr_var_count(const sdfr_renderer *r);
int sdfr_var_info(const sdfr_renderer *r, int index, sdfr_variable *out);
int sdfr_var_set(sdfr_renderer *r, const char *name, float value);
int sdfr_var_get(const sdfr_renderer *r, const char *name, float *out);
int sdfr_vars_reset(sdfr_renderer *r); /* VariableManager::resetVariables: value = start */

/* ---- parameter surface 2: camera + time = the camera constant buffer b0
 *      (SDFRenderer.h:29-34, SDFRenderer.cpp:85-95) and SDFRenderer::setParameters(stime). ---- */
int sdfr_set_camera(sdfr_renderer *r, const float eye[3], const float front[3], const float right[3], const float top[3]);
/* FPS-mode Camera of the reference (Camera.cpp:24-49,156-166): basis from eye -> lookat */
int sdfr_set_camera_lookat(sdfr_renderer *r, const float eye[3], const float lookat[3], float fovy, float aspect, float roll);
int sdfr_set_camera_direction(sdfr_renderer *r, const float eye[3], const float direction[3], float fovy, float aspect, float roll);
int sdfr_get_camera(const sdfr_renderer *r, float out_eye_front_right_top[12]);
int sdfr_set_time(sdfr_renderer *r, float stime);

/* ---- parameter surface 3: the driver's compile-time limits (pshader_sdf.hlsl:60-64,350)
 *      as run-time values.  Defaults = reference; anything else is a labelled extension. ------ */
typedef struct sdfr_limits
{
	int iter_count;       /* ITER_COUNT   100, >= 1 */
	int bounce_count;     /* BOUNCE_COUNT 16, 0..16 */
	int ray_count;        /* RAY_COUNT    8, 1..8 */
	int light_count;      /* LIGHT_COUNT  8, 0..8 */
	float range;          /* RANGE        100 */
	int max_cost_default; /* MaterialOutput.max_cost 7, 0..250 */
	/* EXTENSION, 0 = reference: n = 1..7 point lights orbiting at radius 5, height 3 overwrite slots
	 * 1..n of the scene's map_light table (the "8 lights" variant of the lense/gems benchmark
	 * configuration; the reference's scenes carry one light).  DESIGN.md section 2. */
	int extension_lights;
	/* EXTENSION, 0 = reference: reflection_color given to the labyrinth's marble (MATERIAL_MARBLE_DARK / _LIGHT).
	 * The reference's labyrinth has no reflective material; BASELINE configs[2] is worded "2 reflection bounces":
	 * with 0.25 and the default cost rule (a reflection costs 3 of max_cost 7) a ray is reflected at most twice. */
	float extension_marble_reflection;
	/* the driver's five epsilons, `static const float` in the reference (pshader_sdf.hlsl:31-35), as run-time values.
	 * Defaults = the reference's; anything else is a labelled EXTENSION.
	 *   dist_eps    1e-4  "how close to the object before terminating": the march's hit test (:211), the MATERIAL and
	 *                     OBJECT_TRANSPARENT macros (:80-81), sdSphereFast (sdf_primitives.hlsl:31), the directional
	 *                     light's normalisation (:535); 0 < dist_eps <= 1e-3 (the built-in scenes' culling bounds and
	 *                     escape rules are proved with 0.01 of slack)
	 *   grad_eps    1e-4  spacing of the forward-difference normal samples (:323) -- unless the scene's map_normal sets
	 *                     its own normal_sample_dist; > 0
	 *   reflect_eps 1e-3, refract_eps 1e-3  how far a reflected / refracted ray starts along its direction (:373,397,411); >= 0
	 *   shadow_eps  3e-4  shadow rays start max(shadow_eps, normal_sample_dist) off the surface (:520); >= 0 */
	float dist_eps, grad_eps, reflect_eps, refract_eps, shadow_eps;
} sdfr_limits;
int sdfr_get_limits(const sdfr_renderer *r, sdfr_limits *out);
int sdfr_set_limits(sdfr_renderer *r, const sdfr_limits *limits);

/* how the pipeline stages are scheduled on the GPU (results are identical).  Default: PIXEL,
 * the faster one on every scene measured on MI355X.  WAVEFRONT is kept as a second,
 * differently scheduled implementation for cross-checking (2.7x slower on the headline workload); nothing
 * selects it by itself. */
typedef enum sdfr_schedule
{
	SDFR_SCHEDULE_WAVEFRONT = 0, /* rays in HBM, persistent march waves refilled by ballot, separate shade kernel */
	SDFR_SCHEDULE_PIXEL = 1      /* one lane per pixel, start to finish; pending rays in HBM behind a register cache */
} sdfr_schedule;
int sdfr_set_schedule(sdfr_renderer *r, int schedule);
/* how the PIXEL schedule's kernel is launched (results are identical):
 *   PER_TILE     one single-wave workgroup per 8x8 tile;
 *   PERSISTENT   as many waves as the GPU keeps resident, each pulling tiles from a counter until none is left
 *                (the hardware deals workgroups to its 32 shader engines in strict rotation, so with one
 *                workgroup per tile an engine that draws long-running tiles holds up the others);
 *   AUTO         (default) the scene's own choice: persistent for the built-in scenes with expensive, uneven
 *                tiles, where it measured 2-6 % faster; per tile for the others and for run-time scenes. */
typedef enum sdfr_launch_mode
{
	SDFR_LAUNCH_AUTO = 0,
	SDFR_LAUNCH_PER_TILE = 1,
	SDFR_LAUNCH_PERSISTENT = 2
} sdfr_launch_mode;
int sdfr_set_launch_mode(sdfr_renderer *r, int mode);
/* Step shortcuts (on by default; SDFR_STEP_SHORTCUTS=0 in the environment makes off the default): a ray for which its
   scene can tell that nothing lies ahead any more (cube_sea: above the cubes and not descending) is booked as the miss it
   is going to be without marching its remaining steps.  No pixel and no ray or hit count changes; sdfr_stats.march_evals
   and the per-pixel step counters then fall short of the reference's step counts.  Off: every step is marched, the
   counters equal the reference's (what the parity tests compare).  The reference has no counterpart: it marches on
   (pshader_sdf.hlsl:179-220). */
int sdfr_set_step_shortcuts(sdfr_renderer *r, int enabled);
/* per-round HIP events around the march and shade kernels (sdfr_stats.ms_march / ms_shade); off by default */
int sdfr_set_profiling(sdfr_renderer *r, int enabled);

/* ---- output: the HDR render target SDFRenderer::render draws into
 *      (Application.cpp:274-284; R16G16B16A16_FLOAT, Postprocessing.cpp:23). ------------------ */
typedef enum sdfr_format
{
	SDFR_RGBA32F = 0, /* what the shader computes */
	SDFR_RGBA16F = 1, /* what the reference's render target stores */
	/* strips only (sdfr_render_strips / sdfr_assemble_strips): the RGBA32F frame in 13 bytes per pixel,
	 * lossless -- rgb as three floats, then one byte per pixel for alpha, which is the tone-map flag
	 * (pshader_sdf.hlsl:357-359, 0 or 1).  19 % fewer bytes through the inter-GPU gather; assembles
	 * into an RGBA32F image. */
	SDFR_STRIP_RGB32F_A8 = 2,
	/* strips only: the RGBA16F frame -- what the reference's render target stores (Postprocessing.cpp:23)
	 * -- in 7 bytes per pixel: rgb as three halves (round to nearest even of the fp32 result), then one
	 * byte per pixel for alpha.  Assembles into an RGBA16F image equal, bit for bit, to a direct
	 * SDFR_RGBA16F render.  The smallest wire format: 58 MB per 3840x2160 frame. */
	SDFR_STRIP_RGB16F_A8 = 3
} sdfr_format;

/* Render a width x height frame into `out` (device pointer if out_on_host == 0, else host).
 * pixel_stats (optional, same memory space as `out`): 3 uint32 per pixel = {rays, march
 * evaluations, hits}.  Replaces SDFRenderer::render (SDFRenderer.cpp:65-107). */
int sdfr_render(sdfr_renderer *r, int width, int height, void *out, int format, int out_on_host, uint32_t *pixel_stats);

/* ---- anti-aliasing: supersample and resolve on the device (no counterpart: the reference shoots one ray through each pixel's
 *      centre, pshader_sdf.hlsl:263-267).  K = factor, one of 1, 2, 4, 8.
 *
 *      Let S[Y][X][c], 0 <= Y < K * height, 0 <= X < K * width, be the RGBA32F frame sdfr_render produces at width K * width, height
 *      K * height with the handle's current state: the sub-samples' ray offsets (ddx = 2 / (K * width), ddy = -2 / (K * height)) are
 *      those of that larger frame, which is what supersampling means for the scenes' footprint-filtered materials.  With
 *        box2(A)[y][x][c] = ((A[2y][2x][c] + A[2y][2x+1][c]) + (A[2y+1][2x][c] + A[2y+1][2x+1][c])) * 0.25f
 *      in fp32 and in exactly that order, the image is box2 applied log2 K times to S; K = 1 is S itself.  (A pyramid on purpose:
 *      factor 4 is factor 2 of factor 2.)  S is never held whole: it is rendered and resolved in passes over the strip machinery
 *      below, each pass in a buffer of the handle's own that is kept between calls and freed by sdfr_destroy.
 *        - alpha is averaged like the colours.  It becomes the share of a pixel's sub-samples that carry the tone-map flag, which is
 *          the weight sdfr_postprocess blends the tone-mapped colour with already: an anti-aliased RGBA16F frame goes through it as is.
 *        - format: SDFR_RGBA32F or SDFR_RGBA16F.  The 16F image is the fp32 result converted once, round to nearest even, as a direct
 *          16F render converts its fp32 result -- not an average of halves.  The strip formats: SDFR_ERR_INVALID_ARGUMENT.
 *        - pixel_stats (optional, same memory space as `out`): [height][width][3] uint32, the sums over a pixel's K^2 sub-samples of
 *          {rays, march evaluations, hits}.
 *        - SDFR_ERR_INVALID_ARGUMENT: a factor outside {1, 2, 4, 8}, width or height below 1, K^2 * width * height above 2^30 (the
 *          frame cap of sdfr_render applied to S), a NULL `out`, a bad out_on_host.  SDFR_ERR_NO_SCENE: no scene.  Nothing is written
 *          on error.
 *        - out_on_host = 1 returns with the image there; out_on_host = 0 enqueues every pass on the handle's stream and returns: no
 *          host synchronisation between passes.  With two frames in flight the call runs on the lane of the frame submitted last, as
 *          sdfr_render_strips and sdfr_postprocess do.
 *        - sdfr_get_stats / sdfr_get_timings afterwards report the whole anti-aliased frame: pixels = K^2 * width * height; rays,
 *          evaluations and hits summed over all passes; ms_gpu from the first pass's start to the last resolve's end.  With
 *          sdfr_set_profiling the timings add "draw: resolve", the time inside the resolve launches.
 *        - the handle's strip split (sdfr_set_strip_split) is ignored, as a full frame ignores it.  Built-in and run-time scenes,
 *          both schedules. */
int sdfr_render_aa(sdfr_renderer *r, int width, int height, int factor, void *out, int format, int out_on_host, uint32_t *pixel_stats);

/* A host that renders into host memory (out_on_host = 1) every frame: register the image buffer once.  It is
 * page-locked with the HIP runtime, so the copy of a frame runs at PCIe speed (3840x2160 RGBA32F: ~3 ms) instead
 * of through pageable staging (~12 ms).  The caller keeps the buffer alive and at this address until it registers
 * another one, passes NULL (unregister) or destroys the handle.  Other host destinations keep working, slower. */
int sdfr_register_host_target(sdfr_renderer *r, void *host_image, size_t bytes);

/* Multi-GPU: the frame is cut into strips of SDFR_STRIP_ROWS rows; strip s belongs to rank
 * s % world.  sdfr_render_strips renders this rank's strips into a compact buffer
 * (sdfr_strip_buffer_pixels pixels, strips in increasing order); sdfr_assemble_strips, on the
 * root, scatters a gathered [world][strip_buffer_pixels] array into the full image.  The
 * reference is single-GPU; this is the sharding of SURVEY.md 8(e). */
#define SDFR_STRIP_ROWS 8
int64_t sdfr_strip_buffer_pixels(int width, int height, int world);
int64_t sdfr_strip_buffer_bytes(int width, int height, int world, int format); /* bytes of one rank's compact buffer */
/* Unequal shares: the root's own pixels never cross a link, so when the links into the root bound the
 * frame rate the root should render more than 1 / world of it.  Of every `priv_period` consecutive
 * strips the first `priv_count` (0 <= priv_count < priv_period; 0 = off, the default) are PRIVATE
 * to the root, which renders them straight into the final image with sdfr_render_private_strips;
 * only the others are dealt round-robin, rendered into compact buffers and gathered.  Set the same
 * split on every rank's handle; it applies to sdfr_render_strips and sdfr_assemble_strips
 * (assembly leaves the private rows alone).  The _split variants size the compact buffers. */
int sdfr_set_strip_split(sdfr_renderer *r, int priv_count, int priv_period);
int64_t sdfr_strip_buffer_pixels_split(int width, int height, int world, int priv_count, int priv_period);
int64_t sdfr_strip_buffer_bytes_split(int width, int height, int world, int format, int priv_count, int priv_period);
int sdfr_render_private_strips(sdfr_renderer *r, int width, int height, void *out_image, int format);
int sdfr_render_strips(sdfr_renderer *r, int width, int height, int rank, int world, void *out_compact, int format);
int sdfr_assemble_strips(sdfr_renderer *r, int width, int height, int world, const void *gathered, void *out_image, int format);

/* ---- multi-GPU in the library itself: RCCL over xGMI (no reference counterpart --
 *      the reference drives one adapter, Graphics.cpp:34).  One communicator per process and GPU
 *      (sdfr_comm_create, from an id made on rank 0 and handed to the others by the caller's own
 *      means), or one per device of a single process (sdfr_comm_create_all).  librccl.so is opened
 *      on first use: the library has no load-time dependency on it.
 *
 *      sdfr_render_gather: every rank renders the shared strips of its rank (strip layout above, the
 *      handle's strip split included) in `wire_format` into a buffer the handle owns; the peers
 *      ncclSend theirs to rank 0, which ncclRecv's them (one group per frame, N - 1 messages on N - 1
 *      different xGMI links), scatters them into `root_image` and -- with a strip split -- renders its
 *      private strips straight into `root_image` meanwhile.  Transfer and assembly run on a stream of
 *      the handle's own; the call returns once everything is enqueued and the handle's stream is made
 *      to wait for it, so sdfr_sync (or any later work on that stream) sees the finished image.
 *        image_format SDFR_RGBA32F needs a 32-bit wire format (SDFR_RGBA32F, SDFR_STRIP_RGB32F_A8),
 *        image_format SDFR_RGBA16F a 16-bit one (SDFR_RGBA16F, SDFR_STRIP_RGB16F_A8);
 *        root_image is ignored on the other ranks (may be NULL).
 *      Every rank must call it with the same frame size, formats, strip split, and in the same order
 *      when several handles share one communicator (two frames in flight: two handles, two streams).
 *      sdfr_get_stats afterwards reports this rank's own share. -------------------------------------- */
typedef struct sdfr_comm sdfr_comm;
#define SDFR_COMM_ID_BYTES 128
int sdfr_comm_unique_id(void *id_out);                      /* ncclGetUniqueId; id_out: SDFR_COMM_ID_BYTES bytes */
int sdfr_comm_create(const void *id, int rank, int world, int device_ordinal, sdfr_comm **out); /* collective: ncclCommInitRank */
int sdfr_comm_create_all(const int *device_ordinals, int n, sdfr_comm **out_n);                 /* one process: ncclCommInitAll */
/* Teardown, bounded in time: drains the streams the communicator's transfers ran on (the comm streams of the handles
 * that used it), then ncclCommFinalize + ncclCommDestroy; if that has not finished within SDFR_COMM_CLOSE_TIMEOUT_S
 * (default 30 s) ncclCommAbort is tried and SDFR_ERR_COMM comes back with the call it was stuck in (sdfr_comm_last_error
 * (NULL)) instead of a hang.  Collective in effect: every rank closes.  `c` is gone afterwards either way.
 * sdfr_comm_destroy is the same without the status. */
int sdfr_comm_close(sdfr_comm *c);
void sdfr_comm_destroy(sdfr_comm *c);
/* Which librccl serves this library (path_out, may be NULL), its ncclGetVersion code, and how many DISTINCT librccl files
 * the process maps: more than one means some other component loaded a second copy by path -- a process must not run two
 * (DESIGN.md section 7).  The library itself opens a copy the process already maps (PyTorch's) before any other. */
int sdfr_comm_library_info(char *path_out, size_t path_bytes, int *nccl_version, int *copies_mapped);
int sdfr_comm_rank(const sdfr_comm *c);
int sdfr_comm_world(const sdfr_comm *c);
const char *sdfr_comm_last_error(const sdfr_comm *c);
/* `bytes` bytes travel rank -> (rank + 1) % world -> ... on `hip_stream` (world = 1: to itself) and are
 * compared at the destination: proves that the library, the communicator and the links work.  Blocking and
 * collective: every rank calls it (one process per rank, or one thread per communicator of sdfr_comm_create_all). */
int sdfr_comm_selftest(sdfr_comm *c, size_t bytes, void *hip_stream);
int sdfr_render_gather(sdfr_renderer *r, sdfr_comm *c, int width, int height, void *root_image, int image_format, int wire_format);
/* the same for the n handles / communicators of ONE process (sdfr_comm_create_all), rank i = index i */
int sdfr_render_gather_all(sdfr_renderer *const *r, sdfr_comm *const *c, int n, int width, int height, void *root_image, int image_format,
	int wire_format);

/* ---- the consumer of the render target: HDR::process
 *      (Postprocessing.cpp:130-174; bloom.hlsl; pshader_hdr.hlsl).  scene = the RGBA16F frame of
 *      sdfr_render; bloom_scratch = width*height*8 bytes; out = R8G8B8A8_UNORM (Graphics.cpp:65).
 *      Device pointers; enqueued on the handle's stream. ------------------------------------------ */
int sdfr_postprocess(sdfr_renderer *r, int width, int height, const void *scene_rgba16f, void *bloom_scratch_rgba16f, void *out_rgba8);

int sdfr_sync(sdfr_renderer *r);

/* ---- questions put to the loaded scene (no counterpart: the reference's scene answers only its pixel shader).  Each answer is a
 *      value the reference's driver computes (Engine/shader/pshader_sdf.hlsl), with the handle's current camera, time, variables and
 *      limits latched as sdfr_render latches them; DESIGN.md "Queries".
 *        - on_host = 1: every pointer is host memory and the call returns when the answers are there.  on_host = 0: every pointer is
 *          device memory of the handle's GPU; the work is enqueued on the handle's stream -- with two frames in flight the lane of the
 *          frame submitted last, as sdfr_postprocess -- and the call returns.  With one frame in flight the answers are ready for
 *          work enqueued after the call on the same stream.  With two, that lane's stream is internal and sdfr_wait_frame does not
 *          cover a query (it waits for the frame, which a query never is): call sdfr_sync before reading device answers, or use
 *          on_host = 1.
 *        - n = 0 does nothing; n < 0 or n > INT32_MAX, a NULL required pointer, a bad on_host: SDFR_ERR_INVALID_ARGUMENT; no scene:
 *          SDFR_ERR_NO_SCENE.
 *        - a query changes nothing a render uses or reports: sdfr_get_stats / sdfr_get_timings, the frame sdfr_wait_frame waits for
 *          and the persistent launch's row order stay as they were.
 *      Points, rays and pixels are [n][3] float and [n][2] int32 arrays. ----------------------------------------------------------- */

/* distance[i] = map_geometry (:111-135, debug plane and show_objects included) at GeometryInput{pos = points[i], dir = (0,0,0,0),
 * camera_distance = 0, ray offsets 0} with the default MarchingInput -- dir.w = 0: the scenes' direction-free ("slow") methods.
 * normals (NULL: not wanted) [n][3]: the driver's normal there (:164-177, :320-330): map_normal with the NormalOutput preloaded
 * {grad_eps, 0, false}, its normal if it sets use_normal, else normalize of the three forward differences at normal_sample_dist
 * against baseline = distance[i]. */
int sdfr_query_distance(sdfr_renderer *r, int64_t n, const float *points, float *distance, float *normals, int on_host);

/* The first hit along a ray: what the driver does with a primary ray up to its material (:299-353). */
typedef struct sdfr_hit
{
	float t;              /* camera_distance where the march stopped (in units of |dir|) */
	float distance;       /* scene_distance of its last evaluation */
	float pos[3];         /* mad(dir, t, origin) */
	float normal[3];      /* the driver's normal at the hit (:164-177, :320-330), camera_distance = t, baseline = distance; 0 on a miss */
	uint32_t iterations;  /* iter as march_ray leaves it (:179-220) */
	uint32_t material_id; /* map_material's id at the hit (:333-353), MaterialInput{normal, iterations, distance}; 0 on a miss */
	int32_t hit;          /* 1 hit, 0 miss, -1 invalid item (a pick outside the frame) */
	uint32_t reserved;    /* 0 */
} sdfr_hit;               /* 48 bytes: three 16-byte stores per item (device arrays aligned to 16 bytes) */

/* march_ray (:179-220) from origins[i] along dirs[i] -- used as given, not normalised, dir.w = 1 --, inside_sign +1, the default
 * MarchingInput, dist_max = max_distance (0: limits.range; negative or not finite: SDFR_ERR_INVALID_ARGUMENT), at most
 * limits.iter_count iterations, camera_distance from 0, ray offsets 0.  A ray that starts inside a solid hits at iteration 0.
 * With step shortcuts on (sdfr_set_step_shortcuts) a miss may end early -- hit = 0 with a smaller t, distance and iterations, as
 * march_evals in sdfr_get_stats --; every field of a hit is the same either way. */
int sdfr_query_rays(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits, int on_host);

/* What is under a pixel: pixel (x, y)'s primary ray of a width x height frame of the current camera (:263-267, its ray offsets the
 * pixel's), marched to limits.range, otherwise as sdfr_query_rays.  A pixel outside the frame gives hit = -1. */
int sdfr_pick(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, int on_host);

/* ---- what the surface looks like at a ray's first hit (DESIGN.md "Surface queries"): the driver's lines between the hit and the
 *      light loop (:333-481), restated as a record.  The surface point is the ray query's: pos, dir, camera_distance = t, the ray's
 *      offsets, the driver's normal, iterations, scene_distance.  After map_material (:333-353): the marble extension
 *      (sdfr_limits.extension_marble_reflection), new_normal (:362), and the material switch (:430-481) with the procedural wood,
 *      marble and fire -- whose view direction is the ray's -- and the debug views.  Nothing is spawned and no light is looked at.
 *      The entries are queries in every respect listed above: on_host, what is latched, the stream, no effect on stats, timings or
 *      the row order, n = 0, the argument errors.  `surfaces` is required; `hits` (NULL: not wanted) gets what sdfr_query_rays /
 *      sdfr_pick give for the same items, bit for bit. ---------------------------------------------------------------------------- */
typedef struct sdfr_surface
{
	uint32_t material_id;    /* material_output.material_id after map_material (:333-353) */
	uint32_t flags;          /* SDFR_SURFACE_USE_HDR: material_output.use_hdr; SDFR_SURFACE_LIT: the driver's use_light after the switch */
	uint32_t max_cost;       /* material_output.max_cost */
	int32_t valid;           /* 1 hit, 0 miss, -1 invalid item (a pixel outside the frame); unless 1, every other word is 0 */
	float albedo[3];         /* the driver's local diffuse_color after the switch: diffuse_color.xyz plus the wood / marble term */
	float alpha;             /* material_output.diffuse_color.w after the switch (fire replaces it) */
	float specular[3];       /* material_output.specular_color.xyz */
	float specular_power;    /* ... .w */
	float emissive[3];       /* material_output.emissive_color */
	float optical_index;     /* material_output.optical_index */
	float unlit[3];          /* the driver's `color` right after the switch, before any light: the heat colour of MATERIAL_ITER (from the
	                            hit's iterations and limits.iter_count - 1), the diffuse of MATERIAL_PLAIN, the two normal views, the debug
	                            plane's colour, the fire's colour; 0 for a lit material */
	float reserved0;         /* 0 */
	float reflection[3];     /* material_output.reflection_color, after the marble extension's line */
	float reserved1;         /* 0 */
	float refraction[3];     /* material_output.refraction_color */
	float reserved2;         /* 0 */
	float shading_normal[3]; /* new_normal = lerp(obj_normal, material_output.normal.xyz, material_output.normal.w) (:362) */
	float reserved3;         /* 0 */
} sdfr_surface;              /* 128 bytes: eight 16-byte stores per item (device arrays aligned to 16 bytes; any other alignment: word stores) */
#define SDFR_SURFACE_USE_HDR 1u
#define SDFR_SURFACE_LIT 2u

/* sdfr_query_rays, and the surface at each hit. */
int sdfr_query_ray_surfaces(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits /* or NULL */,
	sdfr_surface *surfaces, int on_host);

/* sdfr_pick, and the surface under each pixel.  pixels_xy = NULL: the G-buffer of the frame -- every pixel, item y * width + x is pixel
 * (x, y), n must be width * height (else SDFR_ERR_INVALID_ARGUMENT); nothing is uploaded, and a wave takes an 8 x 8 tile of pixels as
 * in a render. */
int sdfr_pick_surfaces(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy /* or NULL */, sdfr_hit *hits /* or NULL */,
	sdfr_surface *surfaces, int on_host);

/* The surface at the vertices of a mesh (sdfr_mesh_extract's positions and normals, or any [n][3] arrays like them).  A scene selects
 * its material where |distance| < limits.dist_eps, and a surface-nets vertex lies a fraction of a cell off the surface: asking the
 * scene AT the vertex finds no material.  So vertex i is looked at from outside, by a ray whose march ends on the surface as the
 * driver's does: origin = positions[i] + reach * normals[i] per component (one multiply, then one add, unfused), dir = -normals[i]
 * as given, max_distance = 2 * reach; otherwise sdfr_query_ray_surfaces.  reach must be finite and > 0 (else
 * SDFR_ERR_INVALID_ARGUMENT); a cell or two is a good value.  A vertex whose ray misses (a degenerate normal, a feature thinner than
 * the lattice resolves) gets valid = 0. */
int sdfr_mesh_surfaces(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits /* or NULL */,
	sdfr_surface *surfaces, int on_host);

/* ---- how the scene's lights fall on a ray's first hit (DESIGN.md "Lighting queries"): the driver's light loop (:505-593) and the life of
 *      the shadow rays it starts (:598-632), restated as records.  An item is a ray as in the surface queries -- a caller's ray, a
 *      pixel's primary ray with its ray offsets, a mesh vertex's ray --, marched as sdfr_query_rays / sdfr_pick march it and continued
 *      on a hit exactly as sdfr_surface is: normal, map_material, the marble extension, new_normal, the material switch.  It is treated
 *      as a PRIMARY ray: depth 0, contribution (1, 1, 1), inside_sign +1.  Nothing but shadow rays is spawned: no reflection, no
 *      refraction, no continuation through a see-through hit, no background.
 *      If the driver's use_light is false (sdfr_surface.flags without SDFR_SURFACE_LIT), `own` is the driver's colour after the switch
 *      (sdfr_surface.unlit) and no light is looked at.  Otherwise, in the driver's order of operations, all fp32:
 *      the light table preloaded unused and zero, ambient_lighting_factor 0.075, the scene's map_light, the extension lights;
 *      view_dir = the ray's direction; shadow_move_distance = max(shadow_eps, normal_sample_dist) + max(0, -scene_distance);
 *      scene_pos = mad(new_normal, shadow_move_distance, pos).  For each slot i < limits.light_count that is used, in slot order:
 *      lighting_dir, distance_to_trace and falloff_factor (directional: pos.xyz / (length + dist_eps), limits.range, 1; point:
 *      scene_pos - pos.xyz normalised by its length, that length - extend, pow(0.1, falloff)); light_color = color * falloff_factor;
 *      color += diffuse_color * light_color * ambient_lighting_factor; light_dot = saturate(dot(-new_normal, lighting_dir));
 *      light_influenced_color = 0 + diffuse_color * light_color * light_dot, then + specular_color.xyz * light_color * specular_factor
 *      with half_vec = -normalize(view_dir + lighting_dir), specular_factor = pow(saturate(dot(new_normal, half_vec)), specular_color.w).
 *      A shadow chain is started iff 0 + 2 < max_cost && light_dot > 0.  The driver's ray queue (limits.ray_count) and bounce budget
 *      (limits.bounce_count) are NOT looked at: the query answers as a pixel whose queue never fills and whose bounces never run out.
 *      Chain: pos = scene_pos, dir = -lighting_dir, range = distance_to_trace, C = light_influenced_color * (1, 1, 1) *
 *      saturate(alpha), depth = 2, has_transparent = false, last_transparent_pos = 0.  Each segment is the driver's turn for a shadow
 *      ray (:299-353): march_ray with is_shadow_pass = true, the chain's has_transparent / last_transparent_pos, dist_max = range, the
 *      item's ray offsets, camera_distance from 0.  A miss: the chain ESCAPES and delivers C.  A hit: the normal (map_normal with
 *      dir.w = 0, else the forward differences against scene_distance) and map_material (+ the marble extension's line); the material
 *      switch is not applied.  If diffuse.w < 1 && depth + 2 < max_cost (the hit's own max_cost): C = ((1 - diffuse.w) * diffuse.xyz)
 *      * C, pos = the hit position, range = range - camera_distance, has_transparent = true, last_transparent_pos = pos, depth += 2,
 *      next segment.  Otherwise the chain is BLOCKED and delivers 0.  A chain is also blocked after its 64th segment hits (the driver
 *      has no such bound; its 8-slot queue and bounce_count end a chain far earlier).
 *      After the loop: color = (color + emissive) * saturate(alpha): that is `own`.
 *      `lit` is the renderer's pixel (sdfr_render, RGBA32F, no supersampling; rgb, bit for bit) when all of these hold: the primary
 *      hit spawns nothing else -- no reflection (reflection 0, or max_cost <= 3), no refraction (refraction 0, or max_cost <= 4) and no
 *      continuation through a see-through hit (alpha >= 1, or max_cost <= 2; lit or unlit material alike) --; every started chain has
 *      exactly one segment, so that the driver pops the shadow rays in slot order; and 1 + popcount(traced_mask) <= limits.bounce_count
 *      and <= limits.ray_count.  Otherwise `lit` is the stated sum and not a pixel.
 *      With step shortcuts on only misses end early, so every record is the same with them on or off.
 *      The entries are queries in every respect listed above: on_host, what is latched, the stream, no effect on stats, timings or
 *      the row order, n = 0, the argument errors.  `lighting` is required; `hits` (NULL: not wanted) gets what sdfr_query_rays /
 *      sdfr_pick give for the same items, bit for bit; `lights` (NULL: not wanted) gets eight samples per item, [n][8]. ------------- */
typedef struct sdfr_lighting
{
	int32_t valid;          /* 1 hit, 0 miss, -1 invalid item (a pixel outside the frame); unless 1, every other word is 0 */
	uint32_t used_mask;     /* bit i: slot i < limits.light_count is used */
	uint32_t traced_mask;   /* bit i: a shadow chain was started for it */
	uint32_t visible_mask;  /* bit i: that chain escaped */
	float own[3];           /* the driver's `color` as defined above: the ambient lines and emissive times saturate(alpha), or the unlit colour */
	float ambient_factor;   /* ambient_lighting_factor after map_light; 0 for an unlit material */
	float direct[3];        /* 0, then + delivered of each escaped chain in slot order, fp32 */
	uint32_t segments;      /* shadow segments marched, all chains */
	float lit[3];           /* (0 + own), then + delivered of each escaped chain in slot order, fp32 */
	float reserved;         /* 0 */
} sdfr_lighting;            /* 64 bytes: four 16-byte stores per item (device arrays aligned to 16 bytes; any other alignment: word stores) */

typedef struct sdfr_light_sample
{
	int32_t state;          /* SDFR_LIGHT_UNUSED (also: slot >= limits.light_count, an unlit material, a miss -- then every word is 0),
	                           SDFR_LIGHT_NO_CHAIN used but no chain started, SDFR_LIGHT_BLOCKED, SDFR_LIGHT_ESCAPED */
	uint32_t flags;         /* SDFR_LIGHT_DIRECTIONAL */
	uint32_t segments;      /* of this slot's chain */
	uint32_t reserved0;     /* 0 */
	float dir[3];           /* lighting_dir */
	float distance;         /* distance_to_trace */
	float color[3];         /* light_color, after the falloff */
	float light_dot;
	float influenced[3];    /* light_influenced_color, unshadowed */
	float specular_factor;
	float delivered[3];     /* what the chain delivered: C of an escaped chain, else 0 */
	float reserved1;        /* 0 */
} sdfr_light_sample;        /* 80 bytes, eight per item: five 16-byte stores each (word stores into an array not aligned to 16 bytes) */
#define SDFR_LIGHT_DIRECTIONAL 1u
#define SDFR_LIGHT_UNUSED 0
#define SDFR_LIGHT_NO_CHAIN 1
#define SDFR_LIGHT_BLOCKED 2
#define SDFR_LIGHT_ESCAPED 3

/* sdfr_query_rays, and the lighting at each hit. */
int sdfr_query_ray_lighting(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits /* or NULL */,
	sdfr_lighting *lighting, sdfr_light_sample *lights /* or NULL */, int on_host);

/* sdfr_pick, and the lighting under each pixel.  pixels_xy = NULL: the whole frame as in sdfr_pick_surfaces -- item y * width + x is
 * pixel (x, y), n must be width * height, a wave takes an 8 x 8 tile of pixels. */
int sdfr_pick_lighting(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy /* or NULL */, sdfr_hit *hits /* or NULL */,
	sdfr_lighting *lighting, sdfr_light_sample *lights /* or NULL */, int on_host);

/* The lighting at the vertices of a mesh: each vertex is looked at along the ray sdfr_mesh_surfaces defines (reach finite and > 0),
 * whose direction -normals[i] is also the view direction of the specular term. */
int sdfr_mesh_lighting(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits /* or NULL */,
	sdfr_lighting *lighting, sdfr_light_sample *lights /* or NULL */, int on_host);

/* ---- ambient occlusion at points, hits and mesh vertices (DESIGN.md "Occlusion queries"; no counterpart in the reference): how much
 *      of the hemisphere above a surface point is blocked within a radius, as an integer mask of which of 64 fixed directions hit
 *      something.  Every bit is fixed: there is no floating-point reduction and no dependence on order.
 *      Directions: a table D[64][3] of fp32 unit vectors, cosine-distributed over the hemisphere z > 0.  For k = 0..63, in double
 *      precision, u = (k + 0.5) / 64, phi = 2 pi frac(k (sqrt 5 - 1) / 2), d = (sqrt u cos phi, sqrt u sin phi, sqrt(1 - u)),
 *      normalised, then rounded to fp32.  The committed table (sdfr_occlusion_dirs.h, hexadecimal literals; sdfr_occlusion_directions
 *      returns it) is the definition, not this formula evaluated by some libm.
 *      Frame: from a normal n, used as given and not normalised: s = copysignf(1, n.z), a = -1 / (s + n.z), b = n.x * n.y * a,
 *      t = (1 + s * n.x * n.x * a, s * b, -s * n.x), u = (b, s + n.y * n.y * a, -n.y); every product and sum a separate fp32
 *      operation, left to right as written, unfused.  World direction k, per component c:
 *      w_k[c] = (t[c] * D[k][0] + u[c] * D[k][1]) + n[c] * D[k][2].
 *      Ray k: origin = p + bias * n per component (one multiply, then one add), dir = w_k, and otherwise exactly sdfr_query_rays with
 *      max_distance = radius: march_ray with dir.w = 1, the default MarchingInput, ray offsets 0, at most limits.iter_count
 *      iterations, the debug plane and show_objects included.  Bit k of the mask is set iff that ray's hit == 1.  Step shortcuts do
 *      not change hits, so the mask is the same with them on or off.
 *      An item whose point or normal has a component that is not finite, or whose normal is (0, 0, 0), gets valid = 0 and no march.
 *      Both entries are queries in every respect listed above: on_host, what is latched, the stream, no effect on stats, timings or
 *      the row order, n = 0, the argument errors.  bias must be finite and >= 0, radius finite and > 0 (else
 *      SDFR_ERR_INVALID_ARGUMENT). -------------------------------------------------------------------------------------------------- */
typedef struct sdfr_occlusion
{
	uint32_t mask_lo, mask_hi; /* bit k of the 64-bit mask: direction k hit within radius */
	uint32_t occluded;         /* popcount of the mask, 0..64; openness = 1 - occluded / 64 */
	int32_t valid;             /* 1 answered; 0 nothing to answer (above; a miss of sdfr_hit_occlusion); -1 an invalid item; unless 1 the other words are 0 */
} sdfr_occlusion;              /* 16 bytes: one 16-byte store per item (word stores into an array not aligned to 16 bytes) */

/* The table D, [64][3].  Needs no handle. */
int sdfr_occlusion_directions(float out[64 * 3]);

/* Item i is (points[i], normals[i]), both [n][3]: sdfr_mesh_extract's two arrays as they are, or any arrays like them.  A surface-nets
 * vertex lies a fraction of a cell off the surface, on either side of it: with a bias of about a cell the rays start outside, where a
 * bias of 0 would start some of them inside the solid and count the surface they came from as an occluder.  For points ON the
 * surface (ray hits) a few dist_eps suffice. */
int sdfr_query_occlusion(sdfr_renderer *r, int64_t n, const float *points, const float *normals, float bias, float radius, sdfr_occlusion *out,
	int on_host);

/* Item i is (hits[i].pos, hits[i].normal) where hits[i].hit == 1; otherwise valid = hits[i].hit (0, or -1 for any other value) with
 * zeros elsewhere.  Takes the hits of sdfr_query_rays, sdfr_pick and the surface queries (the whole-frame G-buffer included) as they
 * are: no primary ray is marched a second time and no workspace is needed.  hits needs only 4-byte alignment. */
int sdfr_hit_occlusion(sdfr_renderer *r, int64_t n, const sdfr_hit *hits, float bias, float radius, sdfr_occlusion *out, int on_host);

/* ---- the loaded scene as a triangle mesh: naive surface nets over a lattice of scene distances (no counterpart in the reference;
 *      DESIGN.md "Mesh extraction").  One vertex per grid cell the surface passes through, one quad (two triangles) per lattice edge
 *      that changes sign: an indexed mesh with shared vertices, closed wherever the surface stays inside the grid.  All arithmetic
 *      is fp32 and unfused, in the order written here, so every number of the mesh is defined exactly.
 *
 *      Lattice point (i, j, k), 0 <= i <= nx ..., is at origin + (float)i * cell per axis: one multiply, then one add.
 *      Distance and inside: D(i, j, k) is what sdfr_query_distance returns at that point; s = D - iso; a point is INSIDE iff s < 0
 *      (NaN is therefore outside).
 *      Active cells: cell (i, j, k), 0 <= i < nx ..., has the corners (i + di, j + dj, k + dk); it is ACTIVE iff at least one corner
 *      is inside and at least one is not.  Active cells get consecutive vertex indices in the order of their linear index
 *      i + nx * (j + ny * k).
 *      Vertex position: visit the cell's 12 edges in this order: the 4 along x with (dj, dk) = (0,0), (1,0), (0,1), (1,1); the 4
 *      along y with (di, dk) in that order; the 4 along z with (di, dj) in that order.  An edge runs from its lower endpoint a to
 *      its upper endpoint b; if exactly one of them is inside, t = s_a / (s_a - s_b) and the crossing is a's position with the edge
 *      axis' coordinate replaced by p_a + t * (p_b - p_a).  Each crossing is added component by component to a running sum, in
 *      that order; the vertex is sum / (float)crossings, three divisions.
 *      Quads: every lattice edge from a point P along axis a to its neighbour that has exactly one endpoint inside, where -- with
 *      (a, b, c) the cyclic axis order (x,y,z), (y,z,x) or (z,x,y) -- P's coordinates on axes b and c are >= 1 and <= n_b - 1,
 *      n_c - 1, so that the four cells around the edge exist.  With C(ob, oc) the cell at P offset by ob, oc on axes b and c, the
 *      quad is the vertices of C(-1,-1), C(0,-1), C(0,0), C(-1,0) in that order when P is inside -- counter-clockwise seen from
 *      outside, its normal towards +a -- and in the reverse order, C(-1,0), C(0,0), C(0,-1), C(-1,-1), when P is outside.  Quad
 *      (q0, q1, q2, q3) becomes the triangles (q0, q1, q2) and (q0, q2, q3).  Quads are ordered by P's linear index
 *      i + (nx + 1) * (j + (ny + 1) * k), then by axis x, y, z.  Edges on the grid's boundary emit nothing: the mesh is open where
 *      the surface leaves the box.
 *      Normals: normals[v] is the normal sdfr_query_distance returns at positions[v] (the driver's map_normal, or forward
 *      differences against the distance at the vertex).
 *
 *        - counts is host memory, required, and filled when the call returns: the call reads the two totals back, so it is
 *          synchronous up to that point.  The arrays are host (on_host = 1) or device (on_host = 0) memory as for the queries; with
 *          device arrays the emit work is enqueued on the stream the queries use (two frames in flight: sdfr_sync before reading).
 *        - if either capacity is smaller than the corresponding count, only counts is written, the arrays are untouched and the
 *          call returns SDFR_OK: compare counts with the capacities.  Capacities 0 with NULL arrays: the counting call.
 *        - SDFR_ERR_INVALID_ARGUMENT: a bad grid (below; origin and iso finite), a NULL grid or counts, a negative capacity, a NULL
 *          array with a non-zero capacity (normals excepted: NULL = not wanted), a bad on_host.  SDFR_ERR_NO_SCENE: no scene.
 *        - like a query, the call latches camera, time, variables and limits into a copy and changes nothing a render uses or
 *          reports.  Its workspace (12 bytes per lattice point) is the handle's own and is given back after a call that needed
 *          more than 64 MiB; such a call with device arrays waits for its emit work before it returns. ------------------------- */
typedef struct sdfr_mesh_grid
{
	float origin[3];    /* lattice point (0,0,0) */
	float cell;         /* edge length of a cell, > 0, finite */
	int32_t nx, ny, nz; /* cells per axis, each 1..1024; (nx+1)(ny+1)(nz+1) <= 2^30 */
	float iso;          /* the surface is distance == iso (0: the scene's surface) */
} sdfr_mesh_grid;
typedef struct sdfr_mesh_counts
{
	int64_t vertices, triangles;
} sdfr_mesh_counts;
int sdfr_mesh_extract(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions /*[v][3]*/,
	float *normals /*[v][3] or NULL*/, uint32_t *indices /*[t][3]*/, sdfr_mesh_counts *counts /*host, required*/, int on_host);
/* GPU time of the last sdfr_mesh_extract's stages in ms -- sample the lattice, classify + prefix sums, emit, normals -- if
 * sdfr_set_profiling was on during it (else SDFR_ERR_INVALID_ARGUMENT); a stage that did not run (a counting call, no normals) is 0.
 * Waits for that work. */
int sdfr_mesh_get_timings(sdfr_renderer *r, double ms[4]);

/* ---- ... with the scene's sharp edges and corners kept (DESIGN.md "Sharp mesh extraction").  sdfr_mesh_extract in every respect but
 *      two: the position of each vertex, and normals[v], which follows because it is the point query's normal at positions[v].  The
 *      lattice and the inside test, the active cells and their order, the quads with their order and winding, the indices and the
 *      counts, the capacity rule and the counting call, the argument errors and their precedence, what is latched, the stream, two
 *      frames in flight, on_host and the workspace are sdfr_mesh_extract's, word for word.  The mesh keeps surface nets' connectivity
 *      (dual contouring's): only the vertices move, onto the planes the scene has where the cell's edges cross its surface.
 *
 *      All arithmetic is fp32; every operation is separate and unfused, in the order written.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *      D(q) is what sdfr_query_distance returns at q.  For an active cell, visit its 12 edges in sdfr_mesh_extract's order, from lower
 *      endpoint a to upper endpoint b; an edge with exactly one endpoint inside yields a crossing:
 *      Refine: lo = 0, hi = 1, s_lo = D_a - iso, s_hi = D_b - iso.  Four times: mid = 0.5f * (lo + hi); q = a's position with the
 *      edge axis' coordinate p_a + mid * (p_b - p_a); s = D(q) - iso; if (s < 0) == (s_lo < 0) then lo = mid, s_lo = s, otherwise
 *      hi = mid, s_hi = s.  Then t = lo + (s_lo / (s_lo - s_hi)) * (hi - lo); if !(t >= lo && t <= hi) (NaN too), t = 0.5f * (lo + hi).
 *      The crossing p_i is a's position with the edge axis' coordinate p_a + t * (p_b - p_a).
 *      Plane: d_i and n_i are the distance and the normal sdfr_query_distance returns at p_i; s_i = d_i - iso.  The crossing
 *      contributes a plane iff all of n_i and s_i are finite and n_i is not (0, 0, 0).
 *      Mass point: m = the running per-component sum of all crossings in edge order, divided by (float)crossings -- surface nets'
 *      formula over the refined crossings.
 *      Normal equations, over the c contributing planes in edge order: b_i = ((n_i.x*(p_i.x - m.x) + n_i.y*(p_i.y - m.y)) +
 *      n_i.z*(p_i.z - m.z)) - s_i; H_kl = the running sum from 0 of n_i[k]*n_i[l], six distinct entries; then H_kk = H_kk +
 *      0x1p-8f * (float)c; g_k = the running sum from 0 of n_i[k]*b_i.
 *      Solve, three steps of conjugate gradients from y = 0: r = g, d = g, rr = dot(r, r).  Up to three times: if !(rr > 0) stop;
 *      Hd_k = (H_k0*d.x + H_k1*d.y) + H_k2*d.z; dHd = dot(d, Hd); if !(dHd > 0) stop; alpha = rr / dHd; y_k = y_k + alpha*d_k;
 *      r_k = r_k - alpha*Hd_k; rr2 = dot(r, r); beta = rr2 / rr; d_k = r_k + beta*d_k; rr = rr2.  With c = 0 nothing runs and y = 0.
 *      Vertex: x = m + y; if any component of x is not finite, x = m.  With h = 0.5f * cell, lo_k the cell's lower lattice coordinate
 *      minus h and hi_k its upper one plus h: x_k = fminf(fmaxf(x_k, lo_k), hi_k).
 *
 *        - a vertex therefore never leaves its own cell by more than half a cell on any axis.  A vertex outside its own cell can in
 *          principle fold a quad: the connectivity is not changed to prevent that.
 *        - 8 scene evaluations per crossing (4 bisection samples, the point query and the 3 samples of its normal), about 40 per
 *          vertex, on top of sdfr_mesh_extract's lattice.
 *        - sdfr_mesh_get_timings keeps its four slots: the sharp vertices are counted in "emit". ------------------------------------- */
int sdfr_mesh_extract_sharp(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions /*[v][3]*/,
	float *normals /*[v][3] or NULL*/, uint32_t *indices /*[t][3]*/, sdfr_mesh_counts *counts /*host, required*/, int on_host);

/* ---- where the surface is: what a lattice holds, and the grid that fits the surface (no counterpart in the reference; DESIGN.md
 *      "Mesh survey and fit").  Every result is an integer, counted exactly: no floating-point reduction, no dependence on order.
 *
 *      sdfr_mesh_survey.  D, s = D - iso, INSIDE, ACTIVE and the quad rule are sdfr_mesh_extract's, word for word, and so are the
 *      grid's limits.  A cell is NEAR iff it is active or some corner has fabsf(s) <= band (NaN is never near and never inside).
 *      active_cells is counts.vertices of sdfr_mesh_extract on the same grid and 2 * quads its counts.triangles; inside_points counts
 *      the lattice points with s < 0; the bounds are inclusive cell indices per axis -- with no such cell lo[a] = n[a] and hi[a] = -1;
 *      face_active counts the active cells with i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1 (a cell may lie on
 *      several): the surface leaves the box there, and sdfr_mesh_extract's mesh is open.
 *
 *        - out is host memory; the call is synchronous, like the counting call: it reads the result back.
 *        - like a query, it latches camera, time, variables and limits into a copy and changes nothing a render uses or reports
 *          (stats, timings, row order; sdfr_mesh_get_timings keeps the last extraction's); it runs on the lane of the frame submitted
 *          last.  Its workspace is the mesh workspace of the handle, of which it needs the lattice alone (4 bytes per lattice point)
 *          and 92 KiB for the result words; it is given back after a call that needed more than 64 MiB.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT for a NULL grid or out ("null pointer"), a grid
 *          sdfr_mesh_extract refuses ("bad mesh grid"), a band that is not finite or < 0; then SDFR_ERR_NO_SCENE.  Nothing is written
 *          on error. ------------------------------------------------------------------------------------------------------------ */
typedef struct sdfr_mesh_survey_result
{
	int64_t active_cells;   /* == counts.vertices of sdfr_mesh_extract on the same grid */
	int64_t quads;          /* 2 * quads == counts.triangles */
	int64_t near_cells;
	int64_t inside_points;  /* lattice points with s < 0 */
	int32_t active_lo[3], active_hi[3]; /* inclusive cell indices; none: lo[a] = n[a], hi[a] = -1 */
	int32_t near_lo[3], near_hi[3];
	int64_t face_active[6]; /* active cells with i == 0, i == nx-1, j == 0, j == ny-1, k == 0, k == nz-1 */
} sdfr_mesh_survey_result;
int sdfr_mesh_survey(sdfr_renderer *r, const sdfr_mesh_grid *grid, float band, sdfr_mesh_survey_result *out /* host */);

/*      sdfr_mesh_fit: shrink a search grid onto the surface, coarse to fine.  `search` is a grid at the TARGET cell size c; it may be
 *      far larger than an extractable grid: n[a] in 1 .. 2^20 (origin, cell, iso finite, cell > 0).  levels L in 0 .. 10 with
 *      cell * 2^L finite, margin m in 0 .. 8.
 *
 *      Start with the window lo = 0, hi = n, in cells of the search grid, hi exclusive.  For l = L, L - 1, ..., 0, with step = 1 << l:
 *      the level grid has origin_l[a] = origin[a] + (float)lo[a] * c (one multiply, then one add, unfused), cell_l = c * (float)step,
 *      n_l[a] = ceil((hi[a] - lo[a]) / step), and the same iso.  If sdfr_mesh_extract would refuse the level grid (more than 1024
 *      cells on an axis, more than 2^30 lattice points, an origin that is no longer finite), stop: SDFR_FIT_TOO_LARGE at this level, with
 *      the window so far.  Otherwise survey it with band_l = 1.75f * cell_l for l >= 1 and band_l = 0 for l = 0, and take the bounds
 *      b of its near cells (l >= 1) or of its active cells (l = 0).  If there are none, stop: SDFR_FIT_EMPTY at this level.  Otherwise,
 *      with g = 1 for l >= 1 and g = m for l = 0: lo'[a] = max(lo[a] + (b_lo[a] - g) * step, 0) and hi'[a] = min(lo[a] + (b_hi[a] + 1 + g)
 *      * step, n[a]).  After level 0 the state is SDFR_FIT_FOUND and the fitted grid is origin[a] + (float)lo[a] * c, cell c,
 *      n = hi - lo, iso: extractable by construction, and a sub-lattice of the search grid's wherever the search lattice's coordinates
 *      are exact (dyadic origin and cell).
 *
 *      Why coarse levels may be trusted: sphere tracing already needs |D - iso| never to exceed the true distance to the
 *      iso-surface.  A coarse cell the surface passes through has every corner within its diagonal, sqrt(3) * cell_l < 1.75 * cell_l,
 *      of the surface, so under that contract every corner has |s| <= band_l and the cell is near: no level drops it.
 *        1. With levels = 0 nothing rests on that contract: the fit is one dense survey of the search grid (which must then be
 *           extractable) and its active bounds.
 *        2. A scene whose distance OVERESTIMATES (a warped or scaled field without a matching divisor) may lose what a coarse level
 *           missed: the window can only shrink.
 *        3. With margin >= 1 the fitted grid's mesh is the search grid's mesh: the same vertices in the same order and the same
 *           quads.  Cropping keeps the order of the linear indices, and every active cell ends up interior, so that no quad is
 *           dropped; where the fit is clamped to the search window, the search grid would have dropped those boundary quads as well.
 *
 *        - out is host memory.  state, level (the level reached), surveys (how many ran), lo and hi (the window) are always filled;
 *          grid is the fitted grid when FOUND and zeros otherwise; last is the last survey that ran, zeros if none did.
 *        - protocol, lane and workspace are sdfr_mesh_survey's; the frame is latched once for all levels.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT for a NULL search or out ("null pointer"), a bad search grid,
 *          bad levels, a bad margin; then SDFR_ERR_NO_SCENE.  Nothing is written on error. ---------------------------------------- */
#define SDFR_FIT_EMPTY 0
#define SDFR_FIT_FOUND 1
#define SDFR_FIT_TOO_LARGE 2
typedef struct sdfr_mesh_fit_result
{
	int32_t state;          /* SDFR_FIT_EMPTY 0, SDFR_FIT_FOUND 1, SDFR_FIT_TOO_LARGE 2 */
	int32_t level, surveys; /* the level reached; surveys run */
	int32_t lo[3], hi[3];   /* the window in cells of the search grid, hi exclusive */
	sdfr_mesh_grid grid;    /* FOUND: the fitted grid; else zeros */
	sdfr_mesh_survey_result last; /* the last survey run; zeros if none */
} sdfr_mesh_fit_result;
int sdfr_mesh_fit(sdfr_renderer *r, const sdfr_mesh_grid *search, int levels, int margin, sdfr_mesh_fit_result *out /* host */);

/* ---- whether the solid is in one piece: its parts and its enclosed voids on a lattice (no counterpart in the reference; DESIGN.md
 *      "Components").  Connected-component labelling of the lattice sdfr_mesh_extract samples.  Every result is an integer -- labels,
 *      counts, bounds -- and every bit of it is fixed by the definition: no dependence on order, on the machine or on the run.
 *
 *      Grid.  The grid is sdfr_mesh_grid with sdfr_mesh_extract's limits: origin, cell and iso finite, cell > 0, 1 .. 1024 cells per
 *      axis, at most 2^30 lattice points; anything else is "bad mesh grid".  Lattice point (i, j, k) has the linear index
 *      x = i + px * (j + py * k), with px = nx + 1, py = ny + 1, pz = nz + 1.  D and s = D - iso are sdfr_mesh_extract's.  A point is
 *      INSIDE iff s < 0, so NaN is not inside (and -0.0 is not < 0).
 *
 *      Components.  Two points are joined iff they are neighbours along a lattice axis (6-connectivity) and are both inside or both
 *      not inside.  A component is a class of the closure of that relation: every point belongs to exactly one, either a SOLID (its
 *      points are inside) or a VOID (they are not).
 *        - a component's root is the smallest linear index among its points;
 *        - the components are numbered 0 .. C - 1 in ascending order of root;
 *        - a component is CLOSED iff none of its points lies on a face of the lattice (i = 0, i = px - 1, j = 0, j = py - 1, k = 0,
 *          k = pz - 1).  A closed solid is a part floating free inside the box; a closed void is an enclosed cavity.
 *      6-connectivity is used for both phases, the solid and the void alike.  Two bodies that touch only across a lattice diagonal
 *      are therefore two solids, and a cavity that touches the outside only across a lattice diagonal counts as closed.
 *
 *      sdfr_components_label labels the loaded scene.  sdfr_components_label_lattice labels a caller's lattice[px * py * pz] of
 *      distances, in host or device memory like the other arrays: it needs no scene and uses only n and iso of the grid, which must
 *      still be a good grid.
 *        - counts is host memory and is required; both calls are synchronous, like the counting call of the mesh.  inside_points
 *          equals sdfr_mesh_survey's on the same grid; largest_solid_points and largest_void_points are 0 when there is no component
 *          of that kind.
 *        - labels may be NULL (not wanted); otherwise it is [px * py * pz], and labels[x] is the number of x's component.  It is
 *          written whenever it is given.
 *        - records [capacity] is filled -- records[c] is component c -- iff counts->components <= capacity.  Otherwise only counts is
 *          written, and labels if given, and the call returns SDFR_OK: the mesh's capacity rule.  Capacity 0 with NULL records is the
 *          counting call.
 *        - like a query, the call latches camera, time, variables and limits into a copy and changes nothing a render uses or
 *          reports (stats, timings, row order; sdfr_mesh_get_timings keeps the last extraction's); it runs on the lane of the frame
 *          submitted last.  Its workspace is the mesh workspace of the handle under its keep rule: 12 bytes per lattice point (8
 *          with the caller's lattice), the prefix sum's block sums, 2 KiB of counts and 40 bytes per component.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT for a NULL grid or counts, and for the second entry a NULL
 *          lattice ("null pointer"); an on_host other than 0 or 1; "bad mesh grid"; a negative capacity; NULL records with a capacity;
 *          then, for the first entry only, SDFR_ERR_NO_SCENE.  Nothing is written on error.
 *      (Both structs are defined first and named after: the tag and the typedef are the same name.) ---------------------------------- */
#define SDFR_COMPONENT_INSIDE 1u        /* flags bit 0: a solid */
#define SDFR_COMPONENT_FACE_SHIFT 8     /* flags bits 8 .. 13: touches the face i = 0, i = px-1, j = 0, j = py-1, k = 0, k = pz-1 */
#define SDFR_COMPONENT_FACES 0x3f00u    /* none of them set: closed */
struct sdfr_component /* 40 bytes, 8-byte aligned */
{
	uint32_t root;   /* the smallest linear index of the component's points */
	uint32_t flags;  /* SDFR_COMPONENT_INSIDE | the faces it touches */
	int64_t points;  /* number of lattice points in the component */
	int32_t lo[3], hi[3]; /* inclusive point indices per axis */
};
typedef struct sdfr_component sdfr_component;
struct sdfr_component_counts /* 64 bytes */
{
	int64_t components;
	int64_t solids;
	int64_t voids;
	int64_t closed_solids;
	int64_t closed_voids;
	int64_t inside_points;        /* == sdfr_mesh_survey's on the same grid */
	int64_t largest_solid_points; /* 0: no solid */
	int64_t largest_void_points;  /* 0: no void */
};
typedef struct sdfr_component_counts sdfr_component_counts;
int sdfr_components_label(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t capacity, sdfr_component *records /*[capacity] or NULL*/,
	uint32_t *labels /*[points] or NULL*/, sdfr_component_counts *counts /*host, required*/, int on_host);
int sdfr_components_label_lattice(sdfr_renderer *r, const sdfr_mesh_grid *grid, const float *lattice /*[points]*/, int64_t capacity,
	sdfr_component *records /*[capacity] or NULL*/, uint32_t *labels /*[points] or NULL*/, sdfr_component_counts *counts /*host, required*/, int on_host);

/* ---- the loaded scene's contours on a stack of planes: marching squares over plane lattices of scene distances, the 2-D sibling of
 *      sdfr_mesh_extract (no counterpart in the reference; DESIGN.md "Slices").  An indexed set of line segments with shared vertices:
 *      one vertex per lattice edge that changes sign, one segment per crossing of a cell.  The planes may have any orientation, and the
 *      lattice is not capped at the mesh's 1024 cells per axis.  All arithmetic is fp32; every operation is separate and unfused, in
 *      the order written here, so every number of the result is defined exactly.
 *
 *      Lattice point (i, j) of layer l, 0 <= i <= nu, 0 <= j <= nv, 0 <= l < layers, is per component c
 *      ((origin[c] + (float)i * du[c]) + (float)j * dv[c]) + (float)l * dw[c]; its linear index is i + (nu + 1) * (j + (nv + 1) * l).
 *      Distance and inside: D is what sdfr_query_distance returns at the point; s = D - iso; a point is INSIDE iff s < 0 (NaN is
 *      therefore outside).
 *      Vertices: one per lattice edge inside a layer that has exactly one endpoint inside.  The u-edge of point (i, j) needs i < nu and
 *      runs to (i + 1, j); its v-edge needs j < nv and runs to (i, j + 1).  With a the lower endpoint and b the upper one,
 *      t = s_a / (s_a - s_b); if !(t >= 0 && t <= 1), t = 0.5f.  positions[v][c] = p_a[c] + t * (p_b[c] - p_a[c]) for all three
 *      components; coords[v] is ((float)i + t, (float)j) for a u-edge and ((float)i, (float)j + t) for a v-edge.  Vertices are ordered
 *      by the linear index of the point that owns the edge; at a point the u-edge comes before the v-edge.
 *      Segments: cell (i, j) of layer l, 0 <= i < nu, 0 <= j < nv, has the corners c0 = (i, j), c1 = (i + 1, j), c2 = (i + 1, j + 1),
 *      c3 = (i, j + 1): counter-clockwise in (u, v).  Side k runs from c_k to c_((k + 1) % 4): side 0 is the u-edge of (i, j), side 1
 *      the v-edge of (i + 1, j), side 2 the u-edge of (i, j + 1), side 3 the v-edge of (i, j).  Side k is OUT iff c_k is inside and the
 *      next corner is not, IN iff c_k is not inside and the next corner is; a cell has zero, one or two OUT sides and as many IN sides.
 *      A segment runs from the vertex on an OUT side to the vertex on an IN side: the inside is on its left, and an outer contour
 *      runs counter-clockwise in (u, v).  One OUT side: the one segment.  Two OUT sides (two diagonal corners are inside):
 *      m = ((s0 + s1) + (s2 + s3)) * 0.25f; if m < 0 (NaN is not), OUT side k pairs with IN side (k + 1) % 4, otherwise with IN side
 *      (k + 3) % 4.  The segments of a cell are ordered by OUT side, cells by i + nu * (j + nv * l).  segments[s] is (index of the
 *      start vertex, index of the end vertex).  No segment joins two layers.
 *      Per-layer offsets: layer_vertices[l] is the number of vertices of the layers < l, layer_segments[l] the same for segments;
 *      both have layers + 1 entries, the last being the totals.
 *
 *        - the protocol is sdfr_mesh_extract's, word for word: counts is host memory, required, and filled when the call returns (the
 *          call reads the totals back, so it is synchronous up to that point); the arrays are host (on_host = 1) or device
 *          (on_host = 0) memory, with device arrays the emit work is enqueued on the stream the queries use (two frames in flight:
 *          sdfr_sync before reading); if either capacity is smaller than the corresponding count, only counts and the layer arrays
 *          are written, the arrays are untouched and the call returns SDFR_OK.  Capacities 0 with NULL arrays: the counting call.
 *        - layer_vertices and layer_segments are host memory whatever on_host says, each may be NULL, and they are filled whenever the
 *          call returns SDFR_OK, the counting call included.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT "null pointer" (grid or counts); on_host not 0 or 1; "bad slice
 *          grid" (a non-finite origin, step or iso; du or dv all zero; a count outside its range; more than 2^30 points); a negative
 *          capacity; a NULL array with a non-zero capacity (coords excepted: NULL = not wanted).  Then SDFR_ERR_NO_SCENE.  Nothing is
 *          written on error.
 *        - both totals fit 32 bits (each point and each cell yields at most two); offsets into the arrays are 64-bit.
 *        - like a query, the call latches camera, time, variables and limits into a copy and changes nothing a render uses or
 *          reports: no stats, no timings (sdfr_mesh_get_timings keeps the last mesh extraction's), no row order.  Its workspace, about
 *          12 bytes per lattice point, is sdfr_mesh_extract's under the same keep rule. ---------------------------------------------- */
typedef struct sdfr_slice_grid
{
	float origin[3];        /* lattice point (0,0) of layer 0 */
	float du[3], dv[3];     /* step to the next lattice point along u, along v; finite, neither all zero */
	float dw[3];            /* step from one layer to the next; finite */
	int32_t nu, nv, layers; /* cells per layer 1..16384 each, layers 1..65536; (nu+1)(nv+1)*layers <= 2^30 */
	float iso;              /* the contour is distance == iso (0: the scene's surface) */
} sdfr_slice_grid;
typedef struct sdfr_slice_counts
{
	int64_t vertices, segments;
} sdfr_slice_counts;
int sdfr_slice_extract(sdfr_renderer *r, const sdfr_slice_grid *grid, int64_t vertex_capacity, int64_t segment_capacity, float *positions /*[v][3]*/,
	float *coords /*[v][2] or NULL*/, uint32_t *segments /*[s][2]*/, int64_t *layer_vertices /*[layers+1], host, or NULL*/,
	int64_t *layer_segments /*[layers+1], host, or NULL*/, sdfr_slice_counts *counts /*host, required*/, int on_host);

/* ---- what a ray passes through: the intervals of a ray that lie inside the solid (no counterpart in the reference; DESIGN.md "Spans"),
 *      on the field and with the inside test of sdfr_mesh_extract and sdfr_slice_extract, marched entirely on the GPU.  D is what
 *      sdfr_query_distance returns at a point (the direction-free methods; the debug plane and show_objects apply as they do there); a
 *      point is INSIDE iff D - iso < 0 (NaN is therefore outside).  A span's ends lie on the contours and the mesh, not dist_eps in
 *      front of them.  All arithmetic is fp32; every operation is separate and unfused, in the order written here, so every number of the
 *      result is defined exactly.
 *
 *      Sample: p(t)[c] = origin[c] + t * dir[c], one multiply then one add; s(t) = D(p(t)) - iso; inside iff s < 0.
 *      Start: t_0 = 0.  If the ray is inside at t_0, a span opens with t_in = 0 and SDFR_SPAN_STARTS_INSIDE is set.
 *      Step: a = fabsf(s_i); h = (a > min_step) ? a : min_step (NaN steps by min_step); t' = t_i + h;
 *      t_(i+1) = (t' < t_max) ? t' : t_max; evaluate s_(i+1).
 *      Crossing: if inside differs between the samples i and i + 1, u = s_i / (s_i - s_(i+1)), or 0.5f if !(u >= 0 && u <= 1), and
 *      t* = t_i + u * (t_(i+1) - t_i).  A crossing into the solid opens a span (t_in = t*), a crossing out closes it (t_out = t*).
 *      End: the march ends after the sample at t_max; or, that sample not yet made, after max_steps evaluations, and then
 *      SDFR_SPAN_OUT_OF_STEPS is set (a ray whose max_steps-th sample is the one at t_max is not out of steps).  A span still open is
 *      closed at t_end, the t of the last evaluation, and SDFR_SPAN_ENDS_INSIDE is set.
 *      Storage: span k (0-based, in order) is stored at spans[i * max_spans + k] if k < max_spans; later spans are counted and summed
 *      but not stored.  The slots from min(spans, max_spans) up to max_spans are written as zeros -- all of them for an item without an
 *      answer.  With max_spans = 0, `spans` may be NULL.
 *      Invalid items: if any component of origin or dir is not finite, or dir is (0, 0, 0), the item gets valid = 0 and no evaluation.
 *
 *      What the march rests on: |D - iso| never overestimates the distance to the level set D = iso, outside and inside -- the contract
 *      that sphere tracing, and refraction in the driver, already need.  Under it a sign change can only fall into a step of length
 *      min_step, up to rounding: no feature thicker than min_step along the ray is missed, and a crossing is located to second order in
 *      min_step.  Where a scene breaks the contract the result is still exactly defined by the words above.
 *
 *        - t, t_in and t_out are in units of |dir|: dir is used as given, not normalised, and the steps are taken in t.  A step of h
 *          in t is h * |dir| in space, so the guarantee above is for |dir| <= 1 and the bracket of a crossing is min_step * |dir| long;
 *          pixels' rays have unit length, a mesh's normals should.
 *        - the entries are queries in every respect listed for them: on_host, what is latched, the stream and two frames in flight, no
 *          effect on stats, timings or the row order, n = 0.  n * max(max_spans, 1) <= 2^30.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT "null pointer" (params, summaries, a required input; whatever n
 *          is); on_host not 0 or 1; "bad span parameters"; an item count that is negative or too large; the frame size, or the reach;
 *          a NULL `spans` with max_spans > 0; without a pixel list an n that is not width * height.  Then SDFR_ERR_NO_SCENE.  Nothing
 *          is written on error. -------------------------------------------------------------------------------------------------------- */
typedef struct sdfr_span_params
{
	float t_max;       /* finite, >= 0; 0: limits.range */
	float min_step;    /* finite, > 0 */
	float iso;         /* finite */
	int32_t max_steps; /* 1 .. 1<<20: scene evaluations per item, the one at t = 0 included */
	int32_t max_spans; /* 0 .. 64: spans stored per item */
} sdfr_span_params;
typedef struct sdfr_span
{
	float t_in, t_out;
} sdfr_span; /* 8 bytes; in units of |dir| */
typedef struct sdfr_span_summary
{
	uint32_t crossings;  /* sign changes seen, all of them */
	uint32_t spans;      /* spans opened, all of them; stored = min(spans, max_spans) */
	uint32_t steps;      /* scene evaluations made */
	int32_t valid;       /* 1 answered; 0 nothing to answer; -1 invalid item (a pixel outside the frame); unless 1 all other words 0 */
	float inside_length; /* sum of (t_out - t_in) over ALL spans, in the order they close */
	float t_end;         /* t of the last evaluation */
	uint32_t flags;      /* SDFR_SPAN_* */
	uint32_t reserved;   /* 0 */
} sdfr_span_summary;     /* 32 bytes: two 16-byte stores per item (device arrays aligned to 16 bytes; any other alignment: word stores) */
#define SDFR_SPAN_STARTS_INSIDE 1u
#define SDFR_SPAN_ENDS_INSIDE 2u
#define SDFR_SPAN_OUT_OF_STEPS 4u

/* The spans of rays origins[i] + t * dirs[i], 0 <= t <= t_max. */
int sdfr_query_ray_spans(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, const sdfr_span_params *params,
	sdfr_span_summary *summaries, sdfr_span *spans /* [n][max_spans], or NULL with max_spans = 0 */, int on_host);
/* The spans of pixels' primary rays: the origin and direction sdfr_pick builds for pixel (x, y) of a width x height frame of the current
 * camera.  pixels_xy = NULL: the whole frame in row-major order, n = width * height (a wave takes an 8 x 8 tile).  A pixel outside the
 * frame gets valid = -1. */
int sdfr_pick_spans(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy /* or NULL: the whole frame */,
	const sdfr_span_params *params, sdfr_span_summary *summaries, sdfr_span *spans, int on_host);
/* The spans of sdfr_mesh_surfaces' rays: origin = positions + reach * normals (one multiply, then one add), dir = -normals as given, reach
 * finite and > 0.  The first stored span is then the wall under the vertex, and its length is the thickness there. */
int sdfr_mesh_spans(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, const sdfr_span_params *params,
	sdfr_span_summary *summaries, sdfr_span *spans, int on_host);

/* ---- how much solid there is: volume, centre of mass and inertia of the loaded scene (no counterpart in the reference; DESIGN.md
 *      "Measure"), integrated on the GPU along a bundle of parallel columns and reduced there in a defined order, so that every bit of
 *      the result is defined and only one small record crosses the bus.
 *
 *      A measure grid is nu x nv parallel columns.  Column (i, j), 0 <= i < nu, 0 <= j < nv, is a ray: its origin per component c is
 *      (origin[c] + (float)i * du[c]) + (float)j * dv[c], fp32, one multiply and one add per term (the form of the slices' lattice
 *      points, layer 0); its direction is dw as given.  It is marched exactly as sdfr_query_ray_spans marches that ray under `params`:
 *      the same D, iso, inside test, step rule, crossing rule, end rule and flags; t_max = 0 means limits.range; max_spans must be 0.
 *      The column's spans, steps, crossings, flags and valid below are the words of the sdfr_span_summary of that ray.
 *
 *      Per column, in the order its spans close, with a = (double)t_in, b = (double)t_out, every fp64 operation separate and unfused:
 *        m0 += b - a;   m1 += 0.5 * (b*b - a*a);   m2 += ((b*b)*b - (a*a)*a) / 3.0
 *      -- the integrals of 1, t and t^2 over the inside part of the column; all three start at +0.0.  A column with valid != 1 has
 *      m0 = m1 = m2 = +0.0 and every other word 0.  With u = (double)i and v = (double)j the column's ten contributions are
 *        [m0, u*m0, v*m0, m1, (u*u)*m0, (v*v)*m0, m2, (u*v)*m0, v*m1, u*m1]
 *      and moments[k] is the sum of contribution k over all columns in THIS order:
 *        - the columns of an 8 x 8 tile are lanes l = (i & 7) + 8 * (j & 7); a lane outside the grid, or with valid != 1, is +0.0;
 *        - a tile's value is the pairwise tree over its 64 lanes: level by level x[m] = x[2m] + x[2m + 1];
 *        - tiles are ordered row-major, ti + ceil(nu / 8) * tj;
 *        - then, until one value remains: the values are grouped in runs of 64 by index, the last run padded with +0.0, and each run is
 *          replaced by its pairwise tree sum.  A single tile is its own result.
 *      Exact integers, whatever the order: columns_hit, the columns with spans >= 1; columns_open, those with SDFR_SPAN_STARTS_INSIDE or
 *      SDFR_SPAN_ENDS_INSIDE (the solid leaves the box there: the measure is of a truncated solid); columns_out_of_steps; columns_invalid
 *      (valid != 1); the 64-bit totals of steps, spans and crossings; hit_lo and hit_hi, the inclusive bounds of i ([0]) and j ([1]) over
 *      the hit columns -- with none lo = (nu, nv) and hi = -1, as in the survey; t_lo, the smallest t_in, and t_hi, the largest t_out
 *      over all spans, fp32 -- with no span +inf and -inf.
 *
 *      columns, unless NULL: one 40-byte record per column, row-major i + nu * j, host or device memory as on_host says (device: aligned
 *      to 4 bytes; to 8 for 8-byte stores) -- a mass-per-column or height map in its own right.
 *
 *        - synchronous up to reading `out` back, like the counting call of the mesh; `out` is always host memory.
 *        - a query in every respect listed for the spans: what is latched, the stream and two frames in flight, no effect on stats,
 *          timings or the row order.
 *        - errors, in the order they win: SDFR_ERR_INVALID_ARGUMENT "null pointer" (grid, params, out); on_host not 0 or 1; "bad measure
 *          grid"; "bad span parameters" (max_spans != 0 included); then SDFR_ERR_NO_SCENE.  Nothing is written on error.
 *
 *      sdfr_measure_properties: the physical properties from a result, on the host in fp64, no GPU, every operation separate, in this
 *      order.  A point of the solid is x = origin + u * du + v * dv + t * dw; a column stands for the unit square of (u, v) around it.
 *      With M = moments, A the 3 x 3 matrix whose columns are du, dv, dw (as doubles):
 *        det = (A00 * cx + A10 * cy) + A20 * cz, (cx, cy, cz) = dv x dw = (A11*A22 - A21*A12, A21*A02 - A01*A22, A01*A12 - A11*A02);
 *        volume = M0 * fabs(det); mass = density * volume; cu = M1 / M0, cv = M2 / M0, cw = M3 / M0;
 *        centroid[r] = ((origin[r] + cu * Ar0) + cv * Ar1) + cw * Ar2;
 *        second moments about the lattice centroid, with M0 / 12 for a column's unit footprint: Cuu = (M4 - cu*M1) + M0/12,
 *        Cvv = (M5 - cv*M2) + M0/12, Cww = M6 - cw*M3, Cuv = M7 - cu*M2, Cvw = M8 - cv*M3, Cwu = M9 - cw*M1 (C symmetric);
 *        T = C A^T: Tks = (Ck0*As0 + Ck1*As1) + Ck2*As2;  P = A T: Prs = (Ar0*T0s + Ar1*T1s) + Ar2*T2s;  k = density * fabs(det);
 *        inertia = [k*(Pyy + Pzz), k*(Pzz + Pxx), k*(Pxx + Pyy), -(k*Pxy), -(k*Pyz), -(k*Pzx)]: the tensor about the centroid, world
 *        axes, its off-diagonal elements with their sign.
 *      With !(M0 > 0) it writes zeros and returns SDFR_OK.  NULL pointers or a density that is not finite: SDFR_ERR_INVALID_ARGUMENT. */
typedef struct sdfr_measure_grid
{
	float origin[3];    /* column (0, 0) starts here */
	float du[3], dv[3]; /* step to the next column along u, along v; finite, neither all zero */
	float dw[3];        /* the columns' direction; finite, not all zero */
	int32_t nu, nv;     /* columns per axis, each 1..8192; nu * nv <= 2^24 */
} sdfr_measure_grid;
typedef struct sdfr_measure_result
{
	double moments[10];
	int64_t columns_hit, columns_open, columns_out_of_steps, columns_invalid;
	int64_t steps, spans, crossings;
	int32_t hit_lo[2], hit_hi[2];
	float t_lo, t_hi;
} sdfr_measure_result; /* 160 bytes */
typedef struct sdfr_measure_column
{
	double m0, m1, m2;
	uint32_t spans, steps, flags;
	int32_t valid;
} sdfr_measure_column; /* 40 bytes */
typedef struct sdfr_solid_properties
{
	double volume, mass;
	double centroid[3]; /* world space */
	double inertia[6];  /* about the centroid, world axes: xx, yy, zz, xy, yz, zx */
} sdfr_solid_properties;

int sdfr_measure(sdfr_renderer *r, const sdfr_measure_grid *grid, const sdfr_span_params *params, sdfr_measure_result *out /* host, required */,
	sdfr_measure_column *columns /* [nu * nv], or NULL */, int on_host);
int sdfr_measure_properties(const sdfr_measure_grid *grid, const sdfr_measure_result *res, double density, sdfr_solid_properties *out);

/* ---- a texture atlas of an extracted mesh (no counterpart in the reference; DESIGN.md "Texture atlas"): one square tile of texels per
 *      quad of the mesh, baked on the GPU.  Surface nets emits quads: triangles 2q and 2q + 1 are (q0, q1, q2) and (q0, q2, q3) of one
 *      quad, so a tile per quad needs no chart cutting and no packing search, and bilinear filtering inside a quad never leaves its tile.
 *      All arithmetic is fp32.  Every operation is separate and unfused unless an fma is written.
 *
 *      Layout.  sdfr_atlas_layout(triangles, tile, width, out) is host only and needs no handle.
 *        - tile T is one of 4, 8, 16, 32.
 *        - width W is a multiple of 8 and of T, and W <= 16384.
 *        - triangles is >= 0 and even, and quads = triangles / 2.
 *        - tiles_per_row = W / T.
 *        - rows = ceil(quads / tiles_per_row).
 *        - height H = rows * T rounded up to a multiple of 8, at least 8.
 *        - W * H must be a frame size the renderer accepts (W * H <= 2^30).
 *        - Anything else is SDFR_ERR_INVALID_ARGUMENT.
 *      Quad q owns the tile at column q % tiles_per_row, row q / tiles_per_row.  Its texels are (x0 + a, y0 + b) with x0 = col * T,
 *      y0 = row * T and 0 <= a, b < T.  Texel (x, y) is item y * W + x, and row 0 is the top row of the image.
 *
 *      Quad of a tile.  The quad is (i0, i1, i2, i3) = (idx[2q][0], idx[2q][1], idx[2q][2], idx[2q+1][2]).  The tile is well formed
 *      iff all of these hold:
 *        - idx[2q+1][0] == i0;
 *        - idx[2q+1][1] == i2;
 *        - all four indices are < vertex_count, and the kernel checks this before it loads a vertex.
 *      Otherwise every texel of the tile is invalid (-1).  Texels of no quad are invalid too.  These are the tiles past quads and the
 *      rows past rows * T.
 *
 *      Texel -> surface point.  u = (float)a / (float)(T - 1) and v = (float)b / (float)(T - 1), one division each.  Corners map to
 *      texel centres: q0 <-> (0, 0), q1 <-> (T-1, 0), q2 <-> (T-1, T-1), q3 <-> (0, T-1).  With A any of the two vertex arrays, per
 *      component:
 *        - if u >= v (triangle 2q):  X = (A0 + u * (A1 - A0)) + v * (A2 - A1);
 *        - else (triangle 2q + 1):   X = (A0 + v * (A3 - A0)) + u * (A2 - A3).
 *      P is X of the positions and M is X of the normals.  The unit normal is N = M * r with
 *      r = 1.0f / sqrtf(fmaf(M.z, M.z, fmaf(M.y, M.y, M.x * M.x))).  This is `normalize` of sdfr_math.h as the query unit compiles it,
 *      with IEEE square root and reciprocal.
 *      A texel whose P or M has a non-finite component, or whose M is (0, 0, 0), or whose N is not finite, is DEGENERATE.
 *
 *      UVs.  sdfr_atlas_uvs(atlas, uvs [triangles][3][2], host) is pure host code.  The corner at texel (x, y) gets
 *      (((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H), with the origin top-left.  The corners are in the order of the
 *      triangle's indices.  Bilinear filtering inside a quad never reads another tile.
 *
 *      sdfr_atlas_texels writes, for every texel of the image: valid = 1 with P and N; valid = 0 (degenerate) or -1 (invalid), with
 *      zeros.  This is the escape hatch: a caller runs any existing query over the texels, for example sdfr_query_occlusion for a baked
 *      AO map.  It looks at the mesh alone: it needs NO scene to be loaded and latches nothing; the handle gives the device, the
 *      stream and the staging of a host call.
 *
 *      sdfr_atlas_bake.  A texel with sdfr_atlas_texels valid = 1 is looked at exactly as sdfr_mesh_surfaces / sdfr_mesh_lighting look
 *      at the item (P, N, reach): the ray is theirs, and everything latched is as for a query.  Layers:
 *        SDFR_ATLAS_ALBEDO  (sdfr_surface.albedo where the SDFR_SURFACE_LIT flag is set, else .unlit; .alpha)
 *        SDFR_ATLAS_NORMAL  (sdfr_surface.shading_normal, 0)
 *        SDFR_ATLAS_LIT     (sdfr_lighting.lit, 1)
 *        - Every value is bit for bit that of those records.
 *        - valid = the record's valid, 1 or 0, for a non-degenerate texel of a well-formed tile.  It is 0 for a degenerate texel, which
 *          is not marched, and -1 for an invalid one.
 *        - Every requested plane is written at every texel, with zeros unless valid = 1, so no caller clears anything.
 *        - The lighting part, the light loop and the shadow chains, runs only when SDFR_ATLAS_LIT is asked for.
 *        - reach is finite and > 0, layers is non-zero, and a requested plane's pointer is non-NULL.  Otherwise
 *          SDFR_ERR_INVALID_ARGUMENT.  So is an atlas that sdfr_atlas_layout did not make, and a negative vertex_count.
 *        - on_host, streams, two frames in flight, no effect on stats, timings or the row order, and n = 0 (no triangles: the 8-row
 *          image is filled with -1 and zeros, and no scene is needed) all follow the queries section.  A plane is written by 16-byte
 *          stores into device memory aligned to 16 bytes, by word stores into any other. -------------------------------------------- */
typedef struct sdfr_atlas
{
	int64_t triangles, quads;
	int32_t tile, width, height; /* T, W, H */
	int32_t tiles_per_row, rows;
	int32_t reserved;            /* 0 */
} sdfr_atlas;
#define SDFR_ATLAS_ALBEDO 1u
#define SDFR_ATLAS_NORMAL 2u
#define SDFR_ATLAS_LIT 4u
int sdfr_atlas_layout(int64_t triangles, int tile, int width, sdfr_atlas *out);
int sdfr_atlas_uvs(const sdfr_atlas *atlas, float *uvs /* [triangles][3][2], host */);
int sdfr_atlas_texels(sdfr_renderer *r, const sdfr_atlas *atlas, int64_t vertex_count, const float *positions, const float *normals,
	const uint32_t *indices, float *texel_positions /*[H*W][3]*/, float *texel_normals /*[H*W][3]*/, int32_t *valid /*[H*W]*/, int on_host);
int sdfr_atlas_bake(sdfr_renderer *r, const sdfr_atlas *atlas, int64_t vertex_count, const float *positions, const float *normals,
	const uint32_t *indices, float reach, uint32_t layers, float *albedo, float *normal, float *lit /* each [H*W][4] or NULL */,
	int32_t *valid /* [H*W], required */, int on_host);

/* ---- two frames in flight inside one handle (no counterpart: D3D11's immediate context pipelines the reference's draws by itself)
 *      The end of a frame runs on a nearly empty chip -- the last waves finishing their tiles -- and only the NEXT frame can fill it
 *      (DESIGN.md 4.1).  With n = 2 sdfr_render alternates between two internal streams, each with a workspace of its own (the
 *      memory of the ray queue twice), so that frame k + 1 starts while frame k drains; pixels and counters are those of n = 1.
 *        - sdfr_render returns at once, as always; the frames of one handle may finish out of order.
 *        - the stream given to sdfr_set_stream is not used while n = 2: order other work against a frame with
 *          sdfr_wait_frame(r, stream) -- `stream` waits (on the device, not the host) for the frame submitted last -- or sdfr_sync,
 *          which waits for both frames.  sdfr_get_stats / sdfr_get_timings report the frame submitted last (and wait for it).
 *        - two frames in flight write two buffers: a frame rendered into memory that overlaps the destination of the frame still in
 *          flight (its image or its pixel_stats) waits for that frame first (correct, but nothing overlaps) -- alternate between two images.
 *        - a sdfr_render that fails leaves "the frame submitted last" unchanged: it is still the last frame that succeeded.
 *        - sdfr_render_strips / _gather / sdfr_postprocess run on the lane of the frame submitted last.
 *      n = 1 (the default) returns to one stream (the caller's) after waiting for both frames. ------------------------------------- */
int sdfr_set_frames_in_flight(sdfr_renderer *r, int n);
int sdfr_wait_frame(sdfr_renderer *r, void *hip_stream);

/* ---- observability: GPUProfiler::profile("setup"/"draw") (SDFRenderer.cpp:100,104) ---------- */
typedef struct sdfr_stats
{
	double ms_gpu;          /* HIP-event time of the last render on the handle's stream */
	double ms_march;        /* wavefront schedule: time inside the march kernels */
	double ms_shade;        /* wavefront schedule: time inside the shade kernels */
	uint64_t pixels;
	uint64_t rays;          /* bounce-loop iterations = primary + secondary rays */
	uint64_t march_evals;   /* scene-distance evaluations made while marching */
	uint64_t hits;
	uint32_t march_launches, shade_launches;
} sdfr_stats;
/* waits for the last render, then reports it */
int sdfr_get_stats(sdfr_renderer *r, sdfr_stats *out);

/* ---- named GPU timings: GPUProfiler::profile/getResults (GPUProfiler.h:12-35) with the names the
 *      reference's frame uses ("setup", "draw" SDFRenderer.cpp:100-104; "Bloom 1", "Bloom 2", "HDR"
 *      Postprocessing.cpp:147-171).  "setup" is host time (uniform latch); the vertical blur and
 *      the tone map are one kernel here and report as "Bloom 2 + HDR"; with sdfr_set_profiling the
 *      wavefront schedule adds "draw: march k" / "draw: shade k".  Covers the last sdfr_render* and
 *      the last sdfr_postprocess; waits for them.  Returns the number of entries available (may
 *      exceed `capacity`; only `capacity` are written), or a negative status. ------------------- */
typedef struct sdfr_timing
{
	char name[32];
	double ms;
} sdfr_timing;
int sdfr_get_timings(sdfr_renderer *r, sdfr_timing *out, int capacity);

/* ---- self-test of the kernels' fast exact arithmetic (no reference counterpart) ---------------
 * The kernels replace hipcc's generic correctly rounded fp32 sqrt, and divisions by scene
 * constants, with shorter sequences that give the SAME correctly rounded bits on their stated
 * domain (sdf_playground_amd/csrc/sdfr_math.h: sqrt1, div_c).  This runs the exhaustive
 * comparison on the GPU and returns the number of differing inputs (expected: 0).
 *   what = 0             sqrt1(a)   vs IEEE sqrt   for a = +0 and all a in [2^-96, FLT_MAX]
 *   what = 1, constant c a / c      vs IEEE divide for a = +-0 and all 2^-100 <= |a| <= 2^110
 *   what = 2, constant c negative control: a * (1/c) vs IEEE divide on the same inputs (> 0)
 *   what = 3, constant c as 1 but for a = +-0 and all 2^-60 <= |a| <= 2^40 (fast ground plane) */
int sdfr_selftest_math(sdfr_renderer *r, int what, float constant, uint64_t *mismatches);
/* Throws a C++ exception inside the library the way an allocation failure or a regex error would (what = 0: std::runtime_error,
 * 1: std::bad_alloc, 2: something that is not a std::exception) and returns what the guard at the C boundary makes of it:
 * SDFR_ERR_INTERNAL, with the exception's words in sdfr_last_error(r) when r is not NULL.  Needs no device; r may be NULL. */
int sdfr_selftest_exception(sdfr_renderer *r, int what);

#ifdef __cplusplus
}
#endif
#endif /* SDFR_H */
