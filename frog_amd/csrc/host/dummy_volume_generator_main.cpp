// DummyVolumeGenerator: the empty grid over the group's bounding box that transform.sh reslices every image onto
// (tools/DummyVolumeGenerator.cxx).
//   DummyVolumeGenerator bbox.json spacing
// Writes dummy.mhd + dummy.zraw (float32) in the working directory: origin = bbox[0], `spacing` on every axis,
// dims = ceil((max - min) / spacing).  Upstream leaves the voxels uninitialised; here they are zeros.
#include "frog_host.h"

#include <cstdlib>
#include <iostream>
#include <vector>

int main(int argc, char *argv[])
{
    if (argc < 3) {
        std::cout << "Usage : DummyVolumeGenerator bbox.json spacing" << std::endl;
        exit(-2);
    }
    frog_volume grid;
    if (frog_bbox_grid(argv[1], atof(argv[2]), &grid)) {
        std::cerr << "Error : cannot read a bounding box from " << argv[1] << " (or spacing " << argv[2] << " is not positive)" << std::endl;
        return 1;
    }
    std::vector<float> zeros((size_t)grid.dims[0] * grid.dims[1] * grid.dims[2], 0.0f);
    grid.data = zeros.data();
    if (frog_volume_write("dummy.mhd", &grid)) {
        std::cerr << "Error : cannot write dummy.mhd" << std::endl;
        return 1;
    }
    return 0;
}
