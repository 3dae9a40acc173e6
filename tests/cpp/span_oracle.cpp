// tests/cpp/span_oracle.cpp -- TEST-ONLY: the primary rays of pixels as the CPU oracle's restatement of the reference's driver makes them
// (oracle/driver.h: primary_ray, a step that is called, not restated), for the span tests: sdfr_pick_spans marches the ray sdfr_pick
// builds, and the numpy restatement of the march (tests/span_util.py) needs its origin and direction bit for bit.  The product never
// loads this.
#include "driver.h"
#include "frame_abi.h"

#include <cstdint>

using namespace orc;

extern "C" {

// pixels [n][2] -> origins, dirs [n][3] and valid [n]: 1, or -1 for a pixel outside the frame (its ray stays as the caller left it)
int spo_pixel_rays(const orc_frame *f, int n, const int32_t *pixels, float *origins, float *dirs, int32_t *valid)
{
	const Frame F = enter_frame(*f);
	for (int i = 0; i < n; ++i)
	{
		const int px = pixels[2 * i], py = pixels[2 * i + 1];
		valid[i] = px >= 0 && py >= 0 && px < F.width && py < F.height ? 1 : -1;
		if (valid[i] != 1) continue;
		const PrimaryRay primary = primary_ray(F, px, py);
		origins[3 * i] = val(F.eye.x);
		origins[3 * i + 1] = val(F.eye.y);
		origins[3 * i + 2] = val(F.eye.z);
		dirs[3 * i] = val(primary.dir.x);
		dirs[3 * i + 1] = val(primary.dir.y);
		dirs[3 * i + 2] = val(primary.dir.z);
	}
	return 0;
}
int spo_frame_size() { return (int)sizeof(orc_frame); }

} // extern "C"
