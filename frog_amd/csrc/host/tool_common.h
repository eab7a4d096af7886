// tool_common.h -- what the transform and average tools share: the -t / -ti arguments, the isotropic grid resize, the -b
// background level.
#ifndef FROG_TOOL_COMMON_H
#define FROG_TOOL_COMMON_H

#include "frog_chain.h"
#include "frog_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

extern "C" const char *frog_last_error(void);

// The -t / -ti arguments (tools/PointsTransform.cxx:25-58): how transform files compose into one chain.  The outer
// vtkGeneralTransform is in VTK's default PreMultiply mode, so each file's links go IN FRONT of what is there: of several
// -t/-ti the one given last is applied first.  An inverted file contributes its inverse (reversed links, inverted matrices,
// Newton on the lattices: frog_chain_invert_links); which of -t and -ti that is, is the tool's choice.
struct ChainArguments {
    std::vector<frog_transform_file *> files;       // own the coefficient arrays the links point to
    std::vector<frog_chain_link> links;

    ~ChainArguments() { for (auto *f : files) frog_transform_free(f); }

    // a transform file, owned from here on; null when it cannot be read
    frog_transform_file *read(const char *path)
    {
        int status = 0;
        frog_transform_file *f = frog_transform_read(path, &status);
        if (f) files.push_back(f);
        return f;
    }

    // one -t or -ti argument; on failure `error` holds the message the tools print after "Error : "
    bool add(const char *path, bool inverse, std::string &error)
    {
        frog_transform_file *f = read(path);
        if (!f) { error = std::string("cannot read transform ") + path; return false; }
        const uint32_t n = frog_transform_num_links(f);
        std::vector<frog_chain_link> group(frog_transform_links(f), frog_transform_links(f) + n);
        if (inverse && frog_chain_invert_links(frog_transform_links(f), n, group.data())) { error = frog_last_error(); return false; }
        links.insert(links.begin(), group.begin(), group.end());              // PreMultiply: applied before what is there
        return true;
    }
};

// CheckDiffeomorphism's [spacing], TransformField's -s: the grid resampled to an isotropic spacing over the same extent
// (upstream: vtkImageResize with OutputSpacing), n = max(1, round(n_old * old_spacing / spacing)) nodes per axis from the
// same origin.
inline void resize_isotropic(uint32_t dimensions[3], double spacing[3], double isotropic)
{
    for (int k = 0; k < 3; k++) {
        dimensions[k] = (uint32_t)std::max(1.0, std::floor(dimensions[k] * spacing[k] / isotropic + 0.5));
        spacing[k] = isotropic;
    }
}

// -b backgroundLevel (tools/VolumeTransform.cxx): what a resliced voxel outside the source gets -- the level given, a
// float as upstream parses it, or else the source's minimum
struct BackgroundLevel {
    bool set = false;
    float level = 0;
    void parse(const char *value) { level = atof(value); set = true; }
    double of(double minimum) const { return set ? (double)level : minimum; }
};

#endif
