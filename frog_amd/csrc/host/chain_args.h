// chain_args.h -- the -t / -ti arguments of the transform tools (tools/PointsTransform.cxx:25-58): how transform files
// compose into one chain.  The outer vtkGeneralTransform is in VTK's default PreMultiply mode, so each file's links go IN
// FRONT of what is there: of several -t/-ti the one given last is applied first.  -ti takes the file's inverse (reversed
// links, inverted matrices, Newton on the lattices: frog_chain_invert_links).
#ifndef FROG_CHAIN_ARGS_H
#define FROG_CHAIN_ARGS_H

#include "frog_chain.h"
#include "frog_host.h"

#include <string>
#include <vector>

extern "C" const char *frog_last_error(void);

struct ChainArguments {
    std::vector<frog_transform_file *> files;       // own the coefficient arrays the links point to
    std::vector<frog_chain_link> links;

    // one -t (inverse == false) or -ti argument; on failure `error` holds the message the tools print after "Error : "
    bool add(const char *path, bool inverse, std::string &error)
    {
        int status = 0;
        frog_transform_file *f = frog_transform_read(path, &status);
        if (!f) { error = std::string("cannot read transform ") + path; return false; }
        files.push_back(f);
        const uint32_t n = frog_transform_num_links(f);
        std::vector<frog_chain_link> group(frog_transform_links(f), frog_transform_links(f) + n);
        if (inverse && frog_chain_invert_links(frog_transform_links(f), n, group.data())) { error = frog_last_error(); return false; }
        links.insert(links.begin(), group.begin(), group.end());              // PreMultiply: applied before what is there
        return true;
    }

    ~ChainArguments() { for (auto *f : files) frog_transform_free(f); }
};

#endif
