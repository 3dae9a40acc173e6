// tests/cpp/host_mesh.cpp -- one mesh extraction through the C++ mirror (include/sdfr.hpp: SDFRenderer::extractMesh) from a plain g++
// program: the counting call, then the filling call.
//   host_mesh <scene> <time> <x0> <y0> <z0> <cell> <nx> <ny> <nz> <iso> <out.raw>
// writes counts (2 x int64), positions, normals (float32 [v][3] each) and indices (uint32 [t][3]) to out.raw.
#include "sdfr.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
	if (argc != 12) return 2;
	sdfr::SDFRenderer r;
	if (!r.init(0) || !r.initShader(argv[1]))
	{
		fprintf(stderr, "init failed: %s\n", r.lastError());
		return 1;
	}
	r.setParameters((float)atof(argv[2]));
	sdfr_mesh_grid g;
	for (int a = 0; a < 3; ++a) g.origin[a] = (float)atof(argv[3 + a]);
	g.cell = (float)atof(argv[6]);
	g.nx = atoi(argv[7]);
	g.ny = atoi(argv[8]);
	g.nz = atoi(argv[9]);
	g.iso = (float)atof(argv[10]);
	sdfr_mesh_counts counts = {-1, -1}, again = {-1, -1};
	if (!r.extractMesh(g, 0, 0, nullptr, nullptr, nullptr, counts))
	{
		fprintf(stderr, "counting call failed: %s\n", r.lastError());
		return 1;
	}
	std::vector<float> pos(3 * (size_t)counts.vertices + 1), nrm(3 * (size_t)counts.vertices + 1);
	std::vector<uint32_t> idx(3 * (size_t)counts.triangles + 1);
	if (!r.extractMesh(g, counts.vertices, counts.triangles, pos.data(), nrm.data(), idx.data(), again) || again.vertices != counts.vertices ||
		again.triangles != counts.triangles)
	{
		fprintf(stderr, "filling call failed: %s\n", r.lastError());
		return 1;
	}
	FILE *f = fopen(argv[11], "wb");
	if (!f) return 1;
	fwrite(&counts, sizeof counts, 1, f);
	fwrite(pos.data(), 12, (size_t)counts.vertices, f);
	fwrite(nrm.data(), 12, (size_t)counts.vertices, f);
	fwrite(idx.data(), 12, (size_t)counts.triangles, f);
	fclose(f);
	printf("%lld vertices, %lld triangles\n", (long long)counts.vertices, (long long)counts.triangles);
	return 0;
}
