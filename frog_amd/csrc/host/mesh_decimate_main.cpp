// MeshDecimate: decimation of a triangle mesh by vertex clustering on the GPU (frog_isosurface_upload + frog_isosurface_cluster,
// frog_chain.h; an extension).
//   MeshDecimate source -c cell [-o output.obj] [-dev n]
// One vertex per occupied cell of size `cell` (the units of the points), at the mean of the cell's vertices; a triangle with two
// corners in one cell is dropped, the others keep their order and orientation.  Prints the counts before and after.  Triangles
// only: a mesh with another face is refused.  Input .obj, .ply, .stl or legacy .vtk; output by extension (.obj, .ply, .stl, .vtk,
// .vtp), default output.obj.
#include "tool_common.h"

#include <cstring>
#include <iostream>

int main(int argc, char *argv[])
{
    const char *usage = "Usage : MeshDecimate source -c cell [-o output.obj] [-dev n]";
    if (argc < 4) {
        std::cout << usage << std::endl;
        exit(1);
    }
    const char *outputFile = "output.obj";
    int device = 0;
    bool haveCell = false;
    double cell = 0;
    auto die = [](const std::string &what) { std::cout << "Error : " << what << std::endl; exit(1); };

    int argumentsIndex = 2;
    while (argumentsIndex < argc) {
        char *key = argv[argumentsIndex];
        char *value = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-c") == 0) { cell = atof(value); haveCell = true; }
        if (strcmp(key, "-o") == 0) outputFile = value;
        if (strcmp(key, "-dev") == 0) device = atoi(value);
        argumentsIndex += 2;
    }
    if (!haveCell) die(std::string("-c cell is needed\n") + usage);

    int status = 0;
    frog_mesh_file *file = frog_mesh_read(argv[1], &status);
    if (!file) die(frog_mesh_last_error());
    frog_mesh mesh;
    frog_mesh_view(file, &mesh);
    for (uint32_t f = 0; f < mesh.n_faces; f++)
        if (mesh.face_ptr[f + 1] - mesh.face_ptr[f] != 3)
            die("face " + std::to_string(f) + " has " + std::to_string(mesh.face_ptr[f + 1] - mesh.face_ptr[f]) + " points: MeshDecimate takes triangles only");

    frog_isosurface *surface = nullptr;
    uint32_t nVertices = 0, nTriangles = 0;
    if (frog_isosurface_upload(mesh.xyz, mesh.n_points, mesh.face_idx, mesh.n_faces, device, &surface)) die(frog_last_error());
    if (frog_isosurface_cluster(surface, cell, &nVertices, &nTriangles, nullptr)) die(frog_last_error());
    std::vector<float> xyz(3 * (size_t)nVertices);
    std::vector<uint32_t> triangles(3 * (size_t)nTriangles), facePtr((size_t)nTriangles + 1);
    for (size_t f = 0; f <= nTriangles; f++) facePtr[f] = (uint32_t)(3 * f);
    if (frog_isosurface_get(surface, xyz.data(), triangles.data())) die(frog_last_error());
    frog_isosurface_destroy(surface);
    frog_mesh out = { nVertices, xyz.data(), nTriangles, facePtr.data(), triangles.data() };
    if (frog_mesh_write(outputFile, &out)) die(frog_mesh_last_error());
    std::cout << argv[1] << " : " << mesh.n_points << " vertices, " << mesh.n_faces << " triangles" << std::endl;
    std::cout << outputFile << " : " << nVertices << " vertices, " << nTriangles << " triangles" << std::endl;

    frog_mesh_free(file);
    return 0;
}
