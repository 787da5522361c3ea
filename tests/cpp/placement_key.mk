# host test of the scan order's key function (csrc/placement_key.h), under the address and undefined-behaviour sanitizers:
#   make -C tests/cpp -f placement_key.mk
ROOT := ../..
CXX  ?= g++
all: test_placement_key
test_placement_key: test_placement_key.cpp $(ROOT)/vector_line_quantization_amd/csrc/placement_key.h
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -I$(ROOT)/vector_line_quantization_amd/csrc $< -o $@
clean:
	rm -f test_placement_key
.PHONY: all clean
