# builds the faiss::IndexFlat::range_search shell test against the in-tree library:  make -C tests/cpp -f flat_range.mk
ROOT := ../..
CXX  ?= g++
all: test_flat_range
test_flat_range: test_flat_range.cpp $(wildcard $(ROOT)/include/faiss_amd/*.h) $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O2 -Wall -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I/opt/rocm/include $< -o $@ \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq -Wl,-rpath,'$$ORIGIN/../../vector_line_quantization_amd/csrc' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f test_flat_range
.PHONY: all clean
