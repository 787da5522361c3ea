# builds the faiss::gpu::GpuIndexFlat shell test against the in-tree library:  make -C tests/cpp -f gpuindexflat_shell.mk
ROOT := ../..
CXX  ?= g++
all: test_gpuindexflat_shell
test_gpuindexflat_shell: test_gpuindexflat_shell.cpp $(wildcard $(ROOT)/include/faiss_amd/*.h) $(wildcard $(ROOT)/include/faiss_amd/gpu/*.h) $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O2 -Wall -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I/opt/rocm/include $< -o $@ \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq -Wl,-rpath,'$$ORIGIN/../../vector_line_quantization_amd/csrc' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f test_gpuindexflat_shell
.PHONY: all clean
