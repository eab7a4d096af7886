// TransformField: a FROG transform chain sampled on the voxel grid of a volume, on the GPU: the dense displacement field and
// the map of its Jacobian determinant (frog_chain_sample).  No counterpart among the reference's tools.
//   TransformField reference [-t transform] [-ti inverse_transform] [-s spacing] [-o field.nii.gz] [-j jacobian.nii.gz] [-w chain.json]
// `reference` gives the grid (NIfTI-1 or MetaImage header; the voxels are not read); -s resamples it to an isotropic spacing
// over the same extent by CheckDiffeomorphism's rule, n = max(1, round(n_old * old_spacing / spacing)) nodes per axis from
// the same origin.  -t / -ti compose as in PointsTransform (tool_common.h).  -o writes the field, -j the determinants: NIfTI-1
// FLOAT32 with 3 and 1 components, in the layout of the lattice sidecars.  -w writes a one-entry transform file naming the -o
// file, which the other tools read as a single field link (frog_chain.h); it goes into the directory of the -o file.  The
// headers hold f32 numbers, so a spacing that is no f32 value is stored rounded.  Always prints CheckDiffeomorphism's line
// about negative determinants, then their minimum and maximum.  New: -dev <n> selects the HIP device.
#include "tool_common.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

using std::cout;
using std::endl;

static std::string directory_of(const std::string &path)
{
    const size_t slash = path.find_last_of("/\\");
    return slash == std::string::npos ? std::string(".") : path.substr(0, slash);
}

int main(int argc, char *argv[])
{
    const char *usage = "Usage : TransformField reference [-t transform] [-ti inverse_transform] [-s spacing] [-o field.nii.gz] [-j jacobian.nii.gz] [-w chain.json]";
    if (argc < 2) { cout << usage << endl; return 1; }
    auto die = [](const std::string &what) { cout << "Error : " << what << endl; exit(1); };
    ChainArguments chain;
    std::string error;
    const char *fieldFile = 0, *jacobianFile = 0, *chainFile = 0;
    double resize = 0;
    int device = 0;
    for (int argumentsIndex = 2; argumentsIndex < argc; argumentsIndex += 2) {
        char *key = argv[argumentsIndex];
        char *value = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-t") == 0 || strcmp(key, "-ti") == 0) {
            if (!chain.add(value, strcmp(key, "-ti") == 0, error)) die(error);
        }
        if (strcmp(key, "-s") == 0) resize = atof(value);
        if (strcmp(key, "-o") == 0) fieldFile = value;
        if (strcmp(key, "-j") == 0) jacobianFile = value;
        if (strcmp(key, "-w") == 0) chainFile = value;
        if (strcmp(key, "-dev") == 0) device = atoi(value);
    }
    if (!fieldFile && !jacobianFile) { cout << usage << endl; die("one of -o and -j is needed"); }
    if (chainFile && !fieldFile) die("-w needs the field file of -o");
    if (chainFile && directory_of(chainFile) != directory_of(fieldFile)) die("-w must name a file in the directory of the -o file");

    cout << "load : " << argv[1] << endl;
    uint32_t dimensions[3];
    double origin[3], spacing[3];
    if (frog_volume_geometry(argv[1], dimensions, spacing, origin)) die(std::string("cannot read the grid of ") + argv[1]);
    if (resize > 0) {
        cout << "Resizing image with spacing : " << resize << endl;
        resize_isotropic(dimensions, spacing, resize);
    }
    const size_t n = (size_t)dimensions[0] * dimensions[1] * dimensions[2];

    cout << "Sampling the transform on " << dimensions[0] << " x " << dimensions[1] << " x " << dimensions[2] << " nodes..." << endl;
    // one pass in f64; the files get the f32 cast frog_chain_sample itself would store, the statistics see the f64 values
    std::vector<double> displacement(fieldFile ? 3 * n : 0), determinant(n);
    frog_chain *c = nullptr;
    if (frog_chain_create(chain.links.data(), (uint32_t)chain.links.size(), device, &c)
        || frog_chain_sample(c, origin, spacing, dimensions, FROG_V_F64, fieldFile ? displacement.data() : nullptr, determinant.data()))
        die(frog_last_error());
    frog_chain_destroy(c);

    uint64_t negative = 0;
    double lowest = INFINITY, highest = -INFINITY;
    for (double d : determinant) { negative += d < 0; lowest = std::fmin(lowest, d); highest = std::fmax(highest, d); }
    cout << negative << " negative jacobian determinant values (" << std::setprecision(3)
         << (float)100.0 * negative / ((double)dimensions[0] * dimensions[1] * dimensions[2]) << "%) " << endl;
    cout << std::setprecision(9) << "jacobian determinant range : " << lowest << " " << highest << endl;

    std::vector<float> values;
    if (fieldFile) {
        values.assign(displacement.begin(), displacement.end());
        if (frog_nifti_write(fieldFile, dimensions, spacing, origin, 3, values.data())) { cout << "not able to write  " << fieldFile << endl; return 1; }
        cout << "Field written to " << fieldFile << endl;
    }
    if (jacobianFile) {
        values.assign(determinant.begin(), determinant.end());
        if (frog_nifti_write(jacobianFile, dimensions, spacing, origin, 1, values.data())) { cout << "not able to write  " << jacobianFile << endl; return 1; }
        cout << "Jacobian determinants written to " << jacobianFile << endl;
    }
    if (chainFile) {
        std::string name(fieldFile), escaped;
        const size_t slash = name.find_last_of("/\\");
        if (slash != std::string::npos) name = name.substr(slash + 1);
        for (char ch : name) { if (ch == '"' || ch == '\\') escaped += '\\'; escaped += ch; }
        std::ofstream out(chainFile, std::ios::binary);
        out << "{\"transforms\": [{\"type\": \"frogDisplacementField\", \"file\": \"" << escaped << "\"}]}\n";
        out.close();
        if (!out) { cout << "not able to write  " << chainFile << endl; return 1; }
        cout << "Transform written to " << chainFile << endl;
    }
    return 0;
}
