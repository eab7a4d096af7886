// MeshTransform: a surface mesh through a FROG transform chain, on the GPU (tools/MeshTransform.cxx).
//   MeshTransform source [-t transform] [-ti inverse_transform] [-o outputFileName] [-dev n]
// The points go through frog_chain_apply_f32; the faces, polygons of any size, pass untouched.  -t and -ti compose as in
// PointsTransform (tool_common.h): the outer transform is in VTK's PreMultiply mode, so of several the one given LAST is applied
// to a point FIRST.  Input .obj, .ply, .stl or legacy .vtk; output by extension (.obj, .ply, .stl, .vtk, .vtp), default
// output.obj.  Normals and other point data are not carried.
#include "tool_common.h"

#include <chrono>
#include <cstring>
#include <iostream>

int main(int argc, char *argv[])
{
    if (argc < 3) {
        std::cout << "Usage : MeshTransform source [-t transform] [-ti inverse_transform] [-o outputFileName]" << std::endl;
        exit(1);
    }
    const char *outputFile = "output.obj";
    int device = 0;
    ChainArguments chainArguments;
    std::string error;
    auto die = [](const std::string &what) { std::cout << "Error : " << what << std::endl; exit(1); };
    const auto t0 = std::chrono::steady_clock::now();

    int argumentsIndex = 2;
    while (argumentsIndex < argc) {
        char *key = argv[argumentsIndex];
        char *value = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-t") == 0 || strcmp(key, "-ti") == 0) {
            if (!chainArguments.add(value, strcmp(key, "-ti") == 0, error)) die(error);
        }
        if (strcmp(key, "-o") == 0) outputFile = value;
        if (strcmp(key, "-dev") == 0) device = atoi(value);
        argumentsIndex += 2;
    }

    int status = 0;
    frog_mesh_file *file = frog_mesh_read(argv[1], &status);
    if (!file) die(frog_mesh_last_error());
    frog_mesh mesh;
    frog_mesh_view(file, &mesh);

    frog_chain *chain = nullptr;
    if (frog_chain_create(chainArguments.links.data(), (uint32_t)chainArguments.links.size(), device, &chain)) die(frog_last_error());
    if (frog_chain_apply_f32(chain, mesh.xyz, mesh.xyz, mesh.n_points)) die(frog_last_error());
    if (frog_mesh_write(outputFile, &mesh)) die(frog_mesh_last_error());
    std::cout << "Transform computed in " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s" << std::endl;

    frog_chain_destroy(chain);
    frog_mesh_free(file);
    return 0;
}
