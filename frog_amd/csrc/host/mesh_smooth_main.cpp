// MeshSmooth: Taubin's lambda | mu smoothing of a surface mesh on the GPU (frog_mesh_smooth, frog_chain.h; an extension).
//   MeshSmooth source [-n iterations] [-l lambda] [-m mu] [-b 0|1] [-o output.obj] [-dev n]
// `iterations` times a pass with lambda, then a pass with mu (defaults 20, 0.5, -0.53: no shrinkage to speak of); -l and -m
// equal and positive give the plain Laplacian.  -b 1 (default) lets a border slide along itself, -b 0 pins it.  The faces,
// polygons of any size, pass untouched.  Input .obj, .ply, .stl or legacy .vtk; output by extension (.obj, .ply, .stl, .vtk,
// .vtp), default output.obj.  Normals and other point data are not carried.
#include "tool_common.h"

#include <cstring>
#include <iostream>

int main(int argc, char *argv[])
{
    if (argc < 2) {
        std::cout << "Usage : MeshSmooth source [-n iterations] [-l lambda] [-m mu] [-b 0|1] [-o output.obj] [-dev n]" << std::endl;
        exit(1);
    }
    const char *outputFile = "output.obj";
    int device = 0, boundary = 1;
    long long iterations = 20;
    double lambda = 0.5, mu = -0.53;
    auto die = [](const std::string &what) { std::cout << "Error : " << what << std::endl; exit(1); };

    int argumentsIndex = 2;
    while (argumentsIndex < argc) {
        char *key = argv[argumentsIndex];
        char *value = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-n") == 0) iterations = atoll(value);
        if (strcmp(key, "-l") == 0) lambda = atof(value);
        if (strcmp(key, "-m") == 0) mu = atof(value);
        if (strcmp(key, "-b") == 0) boundary = atoi(value);
        if (strcmp(key, "-o") == 0) outputFile = value;
        if (strcmp(key, "-dev") == 0) device = atoi(value);
        argumentsIndex += 2;
    }
    if (iterations < 0 || iterations > 0x7fffffffLL) die("-n takes a count of iterations");

    int status = 0;
    frog_mesh_file *file = frog_mesh_read(argv[1], &status);
    if (!file) die(frog_mesh_last_error());
    frog_mesh mesh;
    frog_mesh_view(file, &mesh);

    if (frog_mesh_smooth(mesh.xyz, mesh.n_points, mesh.face_ptr, mesh.face_idx, mesh.n_faces, (uint32_t)iterations, lambda, mu, boundary, device))
        die(frog_last_error());
    if (frog_mesh_write(outputFile, &mesh)) die(frog_mesh_last_error());
    std::cout << outputFile << " : " << mesh.n_points << " vertices, " << mesh.n_faces << " faces, " << iterations << " iterations" << std::endl;

    frog_mesh_free(file);
    return 0;
}
