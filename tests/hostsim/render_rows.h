// tests/hostsim/render_rows.h -- TEST-ONLY: the render loop of hostsim.cpp and hlsl_host.cpp.  Threads take the rows of the frame
// one at a time; `pixel(U, x, y, counters, store)` is the product's render_pixel for the scene, with the pixel kernel's store stack.
#pragma once
#include "sdfr_hostframe.h"

#include <atomic>
#include <thread>
#include <vector>

typedef sdfr::CachedRayStore<sdfr::LocalRayStore> HostStore; // same store stack as the pixel kernel

// out_rgba [height][width][4]; out_stats [height][width][3] (rays, march evaluations, hits) or null
template <class PixelFn>
void render_rows(const sdfr::FrameU &U, PixelFn pixel, float *out_rgba, unsigned *out_stats, int nthreads)
{
	std::atomic<int> next_row(0);
	auto worker = [&]() {
		for (;;)
		{
			const int y = next_row.fetch_add(1);
			if (y >= U.height) break;
			for (int x = 0; x < U.width; ++x)
			{
				sdfr::PixelCounters c = {0, 0, 0};
				sdfr::LocalRayStore backing;
				HostStore store(backing);
				const sdfr::vec4 v = pixel(U, x, y, c, store);
				const size_t idx = (size_t)y * U.width + x;
				out_rgba[4 * idx + 0] = v.x;
				out_rgba[4 * idx + 1] = v.y;
				out_rgba[4 * idx + 2] = v.z;
				out_rgba[4 * idx + 3] = v.w;
				if (out_stats)
				{
					out_stats[3 * idx + 0] = c.rays;
					out_stats[3 * idx + 1] = c.march_evals;
					out_stats[3 * idx + 2] = c.hits;
				}
			}
		}
	};
	std::vector<std::thread> pool;
	for (int t = 1; t < nthreads; ++t) pool.emplace_back(worker);
	worker();
	for (auto &th : pool) th.join();
}
