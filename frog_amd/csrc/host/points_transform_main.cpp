// PointsTransform: a point through a FROG transform chain, on the GPU (tools/PointsTransform.cxx).
//   PointsTransform [-p x y z] [-t transform] [-ti inverse_transform] [-o outputFileName]
// -t concatenates a transform file, -ti its inverse (reversed links, inverted matrices, Newton on the
// lattices: frog_chain_invert_links).  The outer vtkGeneralTransform is in VTK's default PreMultiply mode
// (:25-26), so of several -t/-ti the one given LAST is applied to the point FIRST.
#include "tool_common.h"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

using std::cout;
using std::endl;

int main(int argc, char *argv[])
{
    if (argc < 3) {
        std::cout << "Usage : PointsTransform [-p x y z] [-t transform] [-ti inverse_transform] [-o outputFileName]" << std::endl;
        exit(1);
    }
    ChainArguments chain;
    std::string error;
    double *point = 0;
    int argumentsIndex = 1;
    while (argumentsIndex < argc) {
        char *key = argv[argumentsIndex];
        char *value = argumentsIndex + 1 < argc ? argv[argumentsIndex + 1] : (char *)"";
        if (strcmp(key, "-t") == 0 || strcmp(key, "-ti") == 0) {
            if (!chain.add(value, strcmp(key, "-ti") == 0, error)) { cout << "Error : " << error << endl; exit(1); }
        }
        if (strcmp(key, "-p") == 0) {
            if (argumentsIndex + 3 >= argc) { cout << "Error : -p needs three values" << endl; exit(1); }
            point = new double[3];
            for (int i = 0; i < 3; i++) point[i] = atof(argv[argumentsIndex + 1 + i]);
            argumentsIndex += 2;
        }
        argumentsIndex += 2;
    }
    if (point) {
        double newPoint[3];
        cout << "Input point : " << point[0] << " " << point[1] << " " << point[2] << endl;
        frog_chain *c = nullptr;
        if (frog_chain_create(chain.links.data(), (uint32_t)chain.links.size(), 0, &c) || frog_chain_apply(c, point, newPoint, 1)) {
            cout << "Error : " << frog_last_error() << endl;
            exit(1);
        }
        cout << "Output point : " << newPoint[0] << " " << newPoint[1] << " " << newPoint[2] << endl;
        frog_chain_destroy(c);
        delete[] point;
    }
    return 0;
}
