# builds the dump of plan_knn_range (csrc/knn_range_plan.h), host compiler only:  make -C tests/cpp -f knn_range_plan.mk [OUT=path]
ROOT := ../..
CXX  ?= g++
CSRC := $(ROOT)/vector_line_quantization_amd/csrc
OUT  ?= knn_range_plan_dump
all: $(OUT)
$(OUT): knn_range_plan_dump.cpp $(CSRC)/knn_range_plan.h $(CSRC)/knn_plan.h
	$(CXX) -std=c++17 -O1 -Wall -I$(CSRC) $< -o $@
clean:
	rm -f knn_range_plan_dump
.PHONY: all clean
