// IsoSurface: the surface of a scalar volume at a level, or of a label map at a value, as a welded triangle mesh extracted on the
// GPU (frog_isosurface_*, frog_chain.h: marching tetrahedra on the Kuhn decomposition; an extension, the reference makes no mesh).
//   IsoSurface volume (-l level | -v value | -v all) [-s iterations] [-sl lambda] [-sm mu] [-sb 0|1] [-c cell]
//              [-t transform] [-ti inverse_transform] [-o output.obj] [-dev n]
// -l: inside is voxel >= level.  -v: inside is voxel == value (integer volumes).  -v all: one surface per distinct non-zero
// value, ascending, written to <stem>_<value>.<ext> of the output name.  -t / -ti compose as in MeshTransform and are applied to
// the vertices on the device, before the copy back (frog_isosurface_apply).  Output by extension: .obj, .ply, .stl, .vtk, .vtp.
// -s smooths the mesh on the device with Taubin's filter (frog_isosurface_smooth: -sl, -sm and -sb as MeshSmooth's -l, -m and -b,
// defaults 0.5, -0.53, 1), -c decimates it by vertex clustering (frog_isosurface_cluster, as MeshDecimate).  Order: extract,
// smooth, cluster, then -t / -ti, then write; with -v all per value.
#include "tool_common.h"

#include <cstring>
#include <iostream>
#include <set>

template <class S>
static void distinct_values(const frog_volume &v, std::set<long long> &values)
{
    const S *d = (const S *)v.data;
    const size_t n = (size_t)v.dims[0] * v.dims[1] * v.dims[2];
    long long last = 0;
    for (size_t i = 0; i < n; i++) {
        const long long x = (long long)d[i];
        if (x != last) { values.insert(x); last = x; }
    }
    values.erase(0);
}

int main(int argc, char *argv[])
{
    const char *usage = "Usage : IsoSurface volume (-l level | -v value | -v all) [-s iterations] [-sl lambda] [-sm mu] [-sb 0|1] [-c cell] "
                        "[-t transform] [-ti inverse_transform] [-o output.obj] [-dev n]";
    if (argc < 4) {
        std::cout << usage << std::endl;
        exit(1);
    }
    const char *outputFile = "output.obj";
    int device = 0;
    bool haveLevel = false, haveValue = false, all = false;
    double level = 0;
    long long value = 0, smoothIterations = 0;
    double smoothLambda = 0.5, smoothMu = -0.53, cell = 0;
    int smoothBoundary = 1;
    bool haveCell = false;
    ChainArguments chainArguments;
    std::string error;
    auto die = [](const std::string &what) { std::cout << "Error : " << what << std::endl; exit(1); };

    int argumentsIndex = 2;
    while (argumentsIndex < argc) {
        char *key = argv[argumentsIndex];
        char *arg = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-l") == 0) { level = atof(arg); haveLevel = true; }
        if (strcmp(key, "-v") == 0) {
            haveValue = true;
            if (strcmp(arg, "all") == 0) all = true;
            else value = atoll(arg);
        }
        if (strcmp(key, "-t") == 0 || strcmp(key, "-ti") == 0) {
            if (!chainArguments.add(arg, strcmp(key, "-ti") == 0, error)) die(error);
        }
        if (strcmp(key, "-s") == 0) smoothIterations = atoll(arg);
        if (strcmp(key, "-sl") == 0) smoothLambda = atof(arg);
        if (strcmp(key, "-sm") == 0) smoothMu = atof(arg);
        if (strcmp(key, "-sb") == 0) smoothBoundary = atoi(arg);
        if (strcmp(key, "-c") == 0) { cell = atof(arg); haveCell = true; }
        if (strcmp(key, "-o") == 0) outputFile = arg;
        if (strcmp(key, "-dev") == 0) device = atoi(arg);
        argumentsIndex += 2;
    }
    if (smoothIterations < 0 || smoothIterations > 0x7fffffffLL) die("-s takes a count of iterations");
    if (haveLevel == haveValue) die(std::string("one of -l and -v\n") + usage);

    int status = 0;
    frog_volume_file *file = frog_volume_read(argv[1], &status);
    if (!file) die(std::string("cannot read volume ") + argv[1]);
    frog_volume volume;
    frog_volume_view(file, &volume);

    std::set<long long> values;
    if (all) {
        switch (volume.dtype) {
        case FROG_V_U8: distinct_values<uint8_t>(volume, values); break;
        case FROG_V_I8: distinct_values<int8_t>(volume, values); break;
        case FROG_V_U16: distinct_values<uint16_t>(volume, values); break;
        case FROG_V_I16: distinct_values<int16_t>(volume, values); break;
        case FROG_V_U32: distinct_values<uint32_t>(volume, values); break;
        case FROG_V_I32: distinct_values<int32_t>(volume, values); break;
        default: die("-v needs an integer volume");
        }
    } else {
        values.insert(value);           // the one surface of -l or -v
    }

    frog_chain *chain = nullptr;
    if (!chainArguments.links.empty() &&
        frog_chain_create(chainArguments.links.data(), (uint32_t)chainArguments.links.size(), device, &chain)) die(frog_last_error());

    const std::string name(outputFile);
    const size_t dot = name.find_last_of('.'), slash = name.find_last_of('/');
    const bool hasExtension = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    const std::string stem = hasExtension ? name.substr(0, dot) : name, extension = hasExtension ? name.substr(dot) : "";
    std::vector<float> xyz;
    std::vector<uint32_t> triangles, facePtr;
    for (long long v : values) {
        frog_isosurface *surface = nullptr;
        uint32_t nVertices = 0, nTriangles = 0;
        if (frog_isosurface_create(&volume, haveLevel ? FROG_ISO_LEVEL : FROG_ISO_LABEL, level, v, device, &surface, &nVertices, &nTriangles))
            die(frog_last_error());
        if (smoothIterations && frog_isosurface_smooth(surface, (uint32_t)smoothIterations, smoothLambda, smoothMu, smoothBoundary))
            die(frog_last_error());
        if (haveCell && frog_isosurface_cluster(surface, cell, &nVertices, &nTriangles, nullptr)) die(frog_last_error());
        if (chain && frog_isosurface_apply(surface, chain)) die(frog_last_error());
        xyz.resize(3 * (size_t)nVertices);
        triangles.resize(3 * (size_t)nTriangles);
        facePtr.resize((size_t)nTriangles + 1);
        for (size_t f = 0; f <= nTriangles; f++) facePtr[f] = (uint32_t)(3 * f);
        if (frog_isosurface_get(surface, xyz.data(), triangles.data())) die(frog_last_error());
        frog_isosurface_destroy(surface);
        frog_mesh mesh = { nVertices, xyz.data(), nTriangles, facePtr.data(), triangles.data() };
        const std::string path = all ? stem + "_" + std::to_string(v) + extension : name;
        if (frog_mesh_write(path.c_str(), &mesh)) die(frog_mesh_last_error());
        std::cout << path << " : " << nVertices << " vertices, " << nTriangles << " triangles" << std::endl;
    }

    frog_chain_destroy(chain);
    frog_volume_free(file);
    return 0;
}
