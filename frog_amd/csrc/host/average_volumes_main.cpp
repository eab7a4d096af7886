// AverageVolumes: voxel-wise mean and standard deviation of volumes that share one grid (tools/AverageVolumes.cxx), the
// last step of transform.sh, accumulated on the GPU (frog_average, include/frog_chain.h).
//   AverageVolumes f1 ... fN
// Writes average.nii.gz and stdev.nii.gz (float32, the first file's geometry) in the working directory.  Arithmetic as
// upstream's, file order kept: f32 avg += v / N, sq += v * v / N, stdev = sqrt(sq - avg * avg) (NaN where that difference
// rounds negative).  Deviations: sq starts at zero (upstream never clears it) and a file whose dimensions differ from the
// first's is an error (exit 1, nothing written) where upstream reads past its buffer.  Files are read and inflated on host
// threads ahead of the device (volume_stream.h).  New: -dev <n> as the last two arguments selects the HIP device.
#include "group_tool.h"
#include "volume_stream.h"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char *argv[])
{
    int device = 0, n_args = argc;
    if (argc >= 3 && std::strcmp(argv[argc - 2], "-dev") == 0) { device = atoi(argv[argc - 1]); n_args -= 2; }
    if (n_args < 2) {
        std::cout << "Usage : AverageVolumes file1 file2 ... fileN" << std::endl;
        return 1;
    }
    std::vector<std::string> files(argv + 1, argv + n_args);
    static std::thread warm;                        // the HIP runtime comes up while the first file inflates
    warm = std::thread([device] { (void)frog_device_warm(device); });
    std::atexit([] { if (warm.joinable()) warm.join(); });

    int threads;
    size_t window;
    frog::volume_stream_shape(files.size(), &threads, &window);
    frog::VolumeStream stream(files, threads, window);
    frog_average *avg = nullptr;
    frog_volume grid;
    for (size_t i = 0; i < files.size(); i++) {
        std::cout << "load : " << files[i] << std::endl;
        frog::VolumeStream::Item &it = stream.get(i, nullptr);
        if (!it.file) die("cannot read volume " + files[i]);
        if (i == 0) {
            grid = it.view;
            if (frog_average_create(&grid, (uint32_t)files.size(), device, &avg)) die(frog_last_error());
        } else if (std::memcmp(it.view.dims, grid.dims, sizeof grid.dims) != 0) {
            die("dimensions of " + files[i] + " differ from those of " + files[0]);
        }
        if (frog_average_add(avg, nullptr, &it.view, 0, 0.0, nullptr)) die(frog_last_error());
        stream.release(i);
    }
    const size_t total = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    std::vector<float> mean(total), stdev(total);
    if (frog_average_finish(avg, mean.data(), stdev.data())) die(frog_last_error());
    frog_average_destroy(avg);
    grid.dtype = FROG_V_F32;
    grid.data = mean.data();
    if (frog_volume_write("average.nii.gz", &grid)) die("cannot write average.nii.gz");
    grid.data = stdev.data();
    if (frog_volume_write("stdev.nii.gz", &grid)) die("cannot write stdev.nii.gz");
    return 0;
}
